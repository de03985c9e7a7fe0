"""GPU: RDOQ inside the two single-picture residual stages -- kvz_hip_inter_residual_frame_rdoq and kvz_hip_intra_recon_frame_rdoq -- against
tests/golden/rdoq_chain.npz (tests/rdoq_chain_cases.py: every TU from the compiled reference's own kvz_quantize_residual under
cfg.rdoq_enable, a context set per LCU, rdoq_skip on one picture, default scaling lists on another, a tiled run).  Tolerance zero: every
output the chain tests compare, exactly.  Every test runs under a time limit of its own that ends the process, and after a call that
reports a runtime error no further test starts anything on the device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import inter_residual_cases as RC
import lcu_qp_cases as QC
import rdoq_chain_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PICS = {p[0]: p for p in K.PICTURES}
TEST_LIMIT_S = 60
FAULTS = []


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


def _npz(name):
    return np.load(os.path.join(HERE, "golden", name), allow_pickle=False)


@pytest.fixture(scope="module")
def inputs():
    return _npz("lcu_qp.npz")


@pytest.fixture(scope="module")
def golden():
    return _npz("rdoq_chain.npz")


@pytest.fixture(scope="module")
def tables():
    """{0: flat, 1: default} -> (the rdoq tables (quant, err_scale), the scaling tables (quant, dequant) or None)"""
    r, s = _npz("rdoq.npz"), _npz("scaling_list.npz")
    return {0: ((r["quant"][0], r["err_scale"][0]), None), 1: ((r["quant"][1], r["err_scale"][1]), (s["default_quant"], s["default_dequant"]))}


def rdoq_of(api, name, w, h, tables, **over):
    skip, _, lists = K.SETTINGS[name]
    sets, states = K.records(api)
    d = dict(sets=sets, states=states, tables=tables[lists][0], lcu_ctx=K.lcu_ctx_of(name, w, h), skip=skip)
    d.update(over)
    return d


def both(api, pic, case, tables, rdoq, grid=None):
    """the two entries through the numpy wrappers over poisoned outputs (cbf_out cleared) -> (mid, full); rdoq None: the _sl / _tiles /
    _qp entries, {}: the _rdoq entries with rdoq == NULL"""
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes, lcu_qp = case
    scaling = tables[K.SETTINGS[name][2]][1]
    init = QC.zero_outputs(w, h, chroma)
    try:
        mid = api.inter_residual_frame(src, pred, cus, QC.PARAMS_QP, chroma, slice_is_intra, signhide, coeff=init[0], cbf_out=init[1], costs=init[2],
                                       lcu_qp=lcu_qp, scaling=scaling, rdoq=rdoq)
        tiles = api.tile_grid(w, h, *grid) if grid else None
        full = api.intra_recon_frame(src, mid["rec"], mid["cus"], modes, QC.PARAMS_QP, chroma, signhide, slice_is_intra, coeff=mid["coeff"],
                                     cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=lcu_qp, tiles=tiles, scaling=scaling, rdoq=rdoq)
    except Exception:
        FAULTS.append("an _rdoq call")
        raise
    return mid, full


@pytest.mark.parametrize("name", list(PICS))
def test_fixture_through_both_entries(api, inputs, golden, tables, name):
    """rec, coefficients, cus, cbf_out and costs after each stage; the poison outside the owned records stands in the fixture too"""
    pic = PICS[name]
    w, h, chroma = pic[1:4]
    case = K.load_inputs(inputs, pic, golden)
    mid, full = both(api, pic, case, tables, rdoq_of(api, name, w, h, tables))
    RC.assert_outputs_equal(mid, K.load_want(golden, name + "_mid", chroma), "%s inter" % name, chroma)
    RC.assert_outputs_equal(full, K.load_want(golden, name + "_full", chroma), "%s intra" % name, chroma)
    if name == "ragged":                                              # records nobody owns keep the poison, in the fixture as on the device
        assert (K.load_want(golden, name + "_full", chroma)["coeff"][0] == np.int16(RC.POISON_COEFF)).any()


@pytest.mark.parametrize("name", list(PICS))
def test_null_rdoq_is_the_sl_entry(api, inputs, golden, tables, name):
    pic = PICS[name]
    chroma = pic[3]
    case = K.load_inputs(inputs, pic, golden)
    sl_mid, sl_full = both(api, pic, case, tables, None)
    mid, full = both(api, pic, case, tables, {})
    RC.assert_outputs_equal(mid, sl_mid, "%s inter, rdoq == NULL" % name, chroma)
    RC.assert_outputs_equal(full, sl_full, "%s intra, rdoq == NULL" % name, chroma)
    # and RDOQ is not the plain quantiser on this picture
    assert any((a != b).any() for a, b in zip(sl_full["coeff"][:3 if chroma else 1], K.load_want(golden, name + "_full", chroma)["coeff"]))


def test_ragged_with_a_tile_grid(api, inputs, golden, tables):
    pic = PICS["ragged"]
    w, h, chroma = pic[1:4]
    case = K.load_inputs(inputs, pic, golden)
    mid, full = both(api, pic, case, tables, rdoq_of(api, "ragged", w, h, tables), grid=K.TILE_GRID["ragged"])
    RC.assert_outputs_equal(full, K.load_want(golden, "ragged_tiled", chroma), "ragged tiled", chroma)
    assert (K.load_want(golden, "ragged_tiled", chroma)["rec"][0] != K.load_want(golden, "ragged_full", chroma)["rec"][0]).any()


# ---------------------------------------------------------------- the entries on staged device arrays between guard bands
import test_gpu_scaling_list as SLT  # noqa: E402

check = SLT.check
INVALID = SLT.INVALID


def case_dict(pic, case, grid=None):
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes, lcu_qp = case
    col_bd, row_bd = grid if grid else ([0, (w + 63) // 64], [0, (h + 63) // 64])
    return {"name": name, "width": w, "height": h, "chroma": chroma, "src": src, "pred": pred, "cus": cus, "modes": modes, "lcu_qp": lcu_qp,
            "qp": QC.PARAMS_QP, "signhide": signhide, "slice_is_intra": slice_is_intra, "per_lcu": True, "col_bd": col_bd, "row_bd": row_bd,
            "tiled": grid is not None}


class Staged(SLT.Staged):
    """the staging of the scaling-list tests plus what kvz_hip_rdoq_source points at, every array between guard bands"""

    def __init__(self, A, pic, case, tables, pad=0, grid=None):
        from kvazaar_amd import _lib
        name, w, h = pic[:3]
        skip, with_ctx, lists = K.SETTINGS[name]
        SLT.Staged.__init__(self, A, case_dict(pic, case, grid), tables[lists][1], pad=pad)
        sets, states = K.records(A)
        lcu_ctx = K.lcu_ctx_of(name, w, h)
        self.host["sets"], self.host["states"] = [sets], [states]
        self.host["rq_quant"], self.host["rq_err"] = [np.ascontiguousarray(tables[lists][0][0], np.int32)], [np.ascontiguousarray(tables[lists][0][1], np.float64)]
        if lcu_ctx is not None:
            self.host["lcu_ctx"] = [lcu_ctx]
        for k in ("sets", "states", "rq_quant", "rq_err", "lcu_ctx"):
            if k in self.host:
                self.dev[k] = [self._up(self.host[k][0])]
        self.rq = _lib.RdoqSource(self.ptr("sets"), self.ptr("states"), self.ptr("lcu_ctx") if lcu_ctx is not None else None,
                                  _lib.RdoqTables(self.ptr("rq_quant"), self.ptr("rq_err")), len(sets), skip)

    def rq_args(self, over):
        a = self.sl_args(over)
        a.setdefault("rdoq", C.byref(self.rq))
        return a

    def inter_rdoq(self, stream=None, **over):
        a = self.rq_args(over)
        return self.L.kvz_hip_inter_residual_frame_rdoq(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                        a["costs"], a["lcu_qp"], a["tables"], a["rdoq"], a["prm"], stream)

    def intra_rdoq(self, stream=None, **over):
        a = self.rq_args(over)
        return self.L.kvz_hip_intra_recon_frame_rdoq(a["table"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                     a["cbf"], a["costs"], a["lcu_qp"], a["grid"], a["tables"], a["rdoq"], a["prm"], stream)

    def result(self):
        out = SLT.Staged.result(self)
        for k in ("sets", "states", "rq_quant", "rq_err", "lcu_ctx"):
            if k in self.host:
                a = self.host[k][0]
                np.testing.assert_array_equal(self.raw(k, 0)[SLT.TR.GUARD:-SLT.TR.GUARD], a.view(np.uint8).reshape(-1), err_msg=k + " was written")
        return out


def run_both(st, stream=None):
    try:
        check(st.inter_rdoq(stream), "inter_residual_frame_rdoq")
        check(st.intra_rdoq(stream), "intra_recon_frame_rdoq")
    except Exception:
        FAULTS.append("an _rdoq call")
        raise


def test_padded_and_unequal_strides(api, inputs, golden, tables):
    """odd strides, planes that begin three bytes into their rows' padding, the QP array at an odd address; nothing around the picture,
    no guard band and no input is written"""
    pic = PICS["ragged"]
    st = Staged(api, pic, K.load_inputs(inputs, pic, golden), tables, pad=3)
    assert st.host["rec"][0].shape[1] == 207 and st.host["rec"][1].shape[1] == 107 and st.host["src"][0].shape[1] == 207
    run_both(st)
    st.sync()
    RC.assert_outputs_equal(st.result(), K.load_want(golden, "ragged_full", 1), "odd strides", 1)


def test_refusals_on_the_device_write_nothing(api, inputs, golden, tables):
    from kvazaar_amd import _lib
    pic = PICS["coarse"]                                              # with scaling tables: their checks are reached too
    w, h, chroma = pic[1:4]
    case = K.load_inputs(inputs, pic, golden)
    st = Staged(api, pic, case, tables)
    L, good = st.L, st.rq

    def source(**kw):
        f = dict(ctx_sets=good.ctx_sets, states=good.states, lcu_ctx=good.lcu_ctx, quant=good.tables.quant, err_scale=good.tables.err_scale,
                 n_sets=good.n_sets, rdoq_skip=good.rdoq_skip)
        f.update(kw)
        return _lib.RdoqSource(f["ctx_sets"], f["states"], f["lcu_ctx"], _lib.RdoqTables(f["quant"], f["err_scale"]), f["n_sets"], f["rdoq_skip"])
    broken = [source(ctx_sets=None), source(states=None), source(quant=None), source(err_scale=None), source(n_sets=0),
              source(ctx_sets=good.ctx_sets + 1), source(lcu_ctx=good.lcu_ctx + 1), source(states=good.states + 4), source(err_scale=good.tables.err_scale + 4),
              source(quant=good.tables.quant + 8)]
    flat = api.inter_residual_params(QC.PARAMS_QP, 0, 0, chroma, scaling_list=0)
    for call, entry in ((st.inter_rdoq, b"kvz_hip_inter_residual_frame_rdoq"), (st.intra_rdoq, b"kvz_hip_intra_recon_frame_rdoq")):
        for r in broken:
            assert call(rdoq=C.byref(r)) == INVALID, entry
            assert entry in L.kvz_hip_last_error(), L.kvz_hip_last_error()
        # what the _sl entry refuses is refused here too, under this entry's name
        for over in ({"prm": flat.ctypes.data}, {"tables": None}, {"prm": None}, {"table": None}, {"cus": None}, {"cy": st.ptr("coeff", 0) + 2}, {"sy": w - 1}):
            assert call(**over) == INVALID, (entry, sorted(over))
            assert entry in L.kvz_hip_last_error(), (entry, sorted(over), L.kvz_hip_last_error())
    # rdoq == NULL names the _sl entry
    assert st.inter_rdoq(rdoq=None, cus=None) == INVALID and b"kvz_hip_inter_residual_frame_sl" in L.kvz_hip_last_error()
    assert st.intra_rdoq(rdoq=None, cus=None) == INVALID and b"kvz_hip_intra_recon_frame_sl" in L.kvz_hip_last_error()
    st.sync()
    init = QC.zero_outputs(w, h, chroma)
    untouched = {"rec": case[1], "coeff": init[0], "cus": case[2], "cbf_out": init[1], "costs": init[2]}
    RC.assert_outputs_equal(st.result(), untouched, "after refused calls", chroma)
    assert L.kvz_hip_abi_version() == 4


def test_captured_calls_replay_after_the_contents_changed(api, inputs, golden, tables):
    """both entries captured once on `ragged`; replayed after the planes, the outputs, lcu_ctx, the states and the tables were rewritten:
    each replay equals the eager result of the same contents (the fixture, or an eager run of a second staging)"""
    pic = PICS["ragged"]
    w, h, chroma = pic[1:4]
    case = K.load_inputs(inputs, pic, golden)
    st = Staged(api, pic, case, tables)
    L, s, graph = st.L, st.L.kvz_hip_stream_create(), C.c_void_p()
    try:
        check(L.kvz_hip_graph_begin(s), "graph_begin")
        run_both(st, s)
        check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    except Exception:
        FAULTS.append("capture of the _rdoq calls")
        raise
    assert graph.value
    # other contents: the states' lambdas halved, lcu_ctx reversed, the default lists' RDOQ tables, the source planes shifted by one level
    sets, states = K.records(api)
    other_states = np.array(states)
    other_states["lambda"] *= 0.5
    other_ctx = np.ascontiguousarray(st.host["lcu_ctx"][0][::-1])
    other_src = [np.ascontiguousarray(np.clip(p.astype(np.int16) + 1, 0, 255).astype(np.uint8)) for p in st.host["src"]]
    other_tables = (np.ascontiguousarray(tables[1][0][0], np.int32), np.ascontiguousarray(tables[1][0][1], np.float64))
    eager = Staged(api, pic, case, tables)
    for kind, arrs in (("states", [other_states]), ("lcu_ctx", [other_ctx]), ("src", other_src), ("rq_quant", [other_tables[0]]), ("rq_err", [other_tables[1]])):
        for k, a in enumerate(arrs):
            eager.upload(kind, k, a)
            eager.host[kind][k] = a
    run_both(eager)
    eager.sync()
    want_other = eager.result()
    want_first = K.load_want(golden, "ragged_full", chroma)
    assert any((a != b).any() for a, b in zip(want_other["coeff"], want_first["coeff"]))
    first = {k: [np.array(a) for a in st.host[k]] for k in ("states", "lcu_ctx", "src", "rq_quant", "rq_err")}
    other = {"states": [other_states], "lcu_ctx": [other_ctx], "src": other_src, "rq_quant": [other_tables[0]], "rq_err": [other_tables[1]]}
    outputs = {k: [np.array(a) for a in st.host[k]] for k in ("rec", "coeff", "cus", "cbf_out", "costs")}
    try:
        for what, contents, want in (("the first contents", first, want_first), ("other contents", other, want_other), ("the first again", first, want_first)):
            for kind, arrs in list(contents.items()) + list(outputs.items()):
                for k, a in enumerate(arrs):
                    st.upload(kind, k, a, s)
                    st.host[kind][k] = np.ascontiguousarray(a)
            st.sync(s)
            check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            st.sync(s)
            RC.assert_outputs_equal(st.result(), want, "replayed with " + what, chroma)
    except Exception as e:
        if not isinstance(e, AssertionError):
            FAULTS.append("replay of the _rdoq calls")
        raise
    finally:
        L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


def test_inter_stage_against_the_separate_entries(api, inputs, golden, tables):
    """`ragged`: the residual blocks of every inter TU through kvz_hip_transform_batch, then kvz_hip_rdoq_batch with descriptors built from
    the map (type, diagonal scan, CU_INTER, tr_depth of the TU's record, the set of the TU's LCU, a state per (set, QP) pair because the
    batch entry takes the QP from the state) give the stage's coefficient arrays for every TU"""
    pic = PICS["ragged"]
    name, w, h, chroma, signhide, slice_is_intra = pic[:6]
    src, pred, cus, modes, lcu_qp = K.load_inputs(inputs, pic, golden)
    want = K.load_want(golden, "ragged_mid", chroma)
    sets, states = K.records(api)
    lcu_ctx = K.lcu_ctx_of(name, w, h)
    lx = (w + 63) // 64
    pairs, rec_sets, rec_states, descs, blocks, where = {}, [], [], [], [], []
    at = 0
    for (p, x, y, n, cu_x, cu_y) in RC.walk_tus(cus, w, h, chroma):
        sh = 1 if p else 0
        lcu = (y >> 6) * lx + (x >> 6)
        key = (K.set_of(lcu_ctx, lcu), QC.qp_at(lcu_qp, w, x, y))
        if key not in pairs:
            pairs[key] = len(pairs)
            rec_sets.append(sets[key[0]])
            one = states[key[0]:key[0] + 1].copy()                 # a copy of its own: a record taken by index is a view
            one["qp"] = key[1]
            rec_states.append(one[0])
        blk = (slice(y >> sh, (y >> sh) + n), slice(x >> sh, (x >> sh) + n))
        res = src[p][blk].astype(np.int16) - pred[p][blk].astype(np.int16)
        blocks.append((n, res.reshape(-1)))
        d = np.zeros((), dtype=api.RDOQ_DESC)
        d["src_offset"] = d["dst_offset"] = at
        d["width"], d["type"], d["scan_mode"], d["block_type"] = n, 2 if p else 0, 0, api.CU_INTER
        d["tr_depth"], d["ctx_index"] = K.rdoq_tr_depth(cus[y // 4, x // 4]), pairs[key]
        descs.append(d)
        z = RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
        where.append((p, lcu, z, n, at))
        at += n * n
    coef = np.zeros(at, np.int16)
    for n in (4, 8, 16, 32):
        idx = [i for i, b in enumerate(blocks) if b[0] == n]
        if idx:
            out = api.transform_batch("dct", n, np.stack([blocks[i][1] for i in idx]))
            for i, c in zip(idx, out):
                coef[where[i][4]:where[i][4] + n * n] = c
    try:
        levels = api.rdoq_batch(coef, np.array(descs), np.array(rec_sets), np.array(rec_states), tables[0][0], signhide=signhide)
    except Exception:
        FAULTS.append("kvz_hip_rdoq_batch")
        raise
    for (p, lcu, z, n, a) in where:
        np.testing.assert_array_equal(levels[a:a + n * n], want["coeff"][p][lcu, z:z + n * n], err_msg="TU of plane %d width %d in LCU %d at %d" % (p, n, lcu, z))

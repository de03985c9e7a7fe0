"""GPU: kvz_hip_rdoq_batch against tests/golden/rdoq.npz (what the compiled reference's own kvz_rdoq left in dest_coeff): the whole fixture
in one call per configuration, byte for byte; the same TUs shuffled and cut into several calls; further seeded TUs of every width against
the model; skipped descriptors and every error path against a canary fill; a captured call replayed after the contents of coef, descs,
ctx_sets and states changed; TUs addressed as the picture chain lays coefficients out.  Tolerance is zero throughout.  Every test runs
under a time limit of its own that ends the process, and after a call that reports a runtime error no further test starts anything on the
device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import inter_residual_cases as IRC
import rdoq_cases as K
import rdoq_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdoq.npz")
TEST_LIMIT_S = 90
CANARY = 0x5a5a
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


def check(api, rc, what):
    try:
        api.check(rc, what)
    except Exception:
        FAULTS.append(what)
        raise


def make_descs(api, rows):
    """rows of (src_offset, dst_offset, width, type, scan_mode, block_type, tr_depth, set)"""
    descs = np.zeros(len(rows), dtype=api.RDOQ_DESC)
    for i, (src, dst, width, type_, scan, block_type, tr_depth, set_) in enumerate(rows):
        descs[i] = (src, dst, width, type_, scan, block_type, tr_depth, 0, set_)
    return descs


@pytest.fixture(scope="module")
def fx(api):
    """the fixture as the entry takes it: coefficients, descriptors (dest laid out as coef is), the two records of every set, the tables of
    both list kinds, the configuration of every TU and the recorded results"""
    z = np.load(GOLDEN)
    d = z["desc"].astype(np.int64)
    descs = make_descs(api, [(o, o, w, t, s, b, dep, set_) for o, w, t, s, b, dep, set_, _ in d.tolist()])
    sets = np.array([api.coeff_ctx_from_dump(dump, 256) for dump in z["dumps"]], dtype=api.COEFF_CTX)
    states = np.array([api.rdoq_state_from_dump(dump, lam, qp) for dump, lam, qp in zip(z["dumps"], z["lambdas"], z["qps"])], dtype=api.RDOQ_STATE)
    return dict(coeffs=z["coeffs"], descs=descs, sets=sets, states=states, cfg=d[:, 7], configs=[tuple(c) for c in z["configs"].tolist()], dest=z["dest"],
                tables=[(z["quant"][k], z["err_scale"][k]) for k in (0, 1)], dumps=z["dumps"], qps=z["qps"], lambdas=z["lambdas"], d=d)


def run(api, fx, coef, descs, cfg, dest=None, sets=None, states=None):
    signhide, sl = fx["configs"][cfg]
    try:
        return api.rdoq_batch(coef, descs, fx["sets"] if sets is None else sets, fx["states"] if states is None else states, fx["tables"][sl], signhide,
                              dest=dest)
    except Exception:
        FAULTS.append("rdoq_batch")
        raise


def covered(descs, size, field="dst_offset"):
    """bool [size]: the values the descriptors' TUs cover"""
    m = np.zeros(size, dtype=bool)
    for o, w in zip(descs[field].tolist(), descs["width"].tolist()):
        m[o:o + w * w] = True
    return m


def same(got, want, what):
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, "%s: %d of %d values differ, first at %d: got %d, want %d" % (what, wrong.size, len(want), wrong[0], got[wrong[0]], want[wrong[0]])


def test_whole_fixture_in_one_call_per_configuration(api, fx):
    n = fx["coeffs"].size
    for cfg in range(len(fx["configs"])):
        mine = fx["cfg"] == cfg
        assert mine.sum() >= 100
        descs = fx["descs"][mine]
        got = run(api, fx, fx["coeffs"], descs, cfg, dest=np.full(n, CANARY, dtype=np.int16))
        m = covered(descs, n)
        same(got[m], fx["dest"][m], "configuration %r" % (fx["configs"][cfg],))
        assert (got[~m] == CANARY).all()                        # nothing outside the TUs of the call is written


@pytest.mark.parametrize("chunk", (1, 63, 65, 200))
def test_shuffled_and_cut_into_calls(api, fx, chunk):
    g = np.random.default_rng(chunk)
    idx = g.permutation(np.flatnonzero(fx["cfg"] == 0))[:{1: 12, 63: 63 * 3, 65: 65 * 3, 200: 600}[chunk]]
    n = fx["coeffs"].size
    for at in range(0, len(idx), chunk):
        descs = fx["descs"][idx[at:at + chunk]]
        got = run(api, fx, fx["coeffs"], descs, 0, dest=np.full(n, CANARY, dtype=np.int16))
        m = covered(descs, n)
        same(got[m], fx["dest"][m], "TUs %d.. in calls of %d" % (at, chunk))
        assert (got[~m] == CANARY).all()


@pytest.mark.parametrize("width", (4, 8, 16, 32))
def test_seeded_tus_equal_the_model(api, fx, width):
    cs = K.extra_cases(1000 + width, per_width=300, widths=(width,))
    coef, d = K.pack(cs)
    for cfg in range(len(fx["configs"])):
        mine = np.flatnonzero(d[:, 7] == cfg)
        descs = make_descs(api, [(d[i, 0], d[i, 0], *d[i, 1:7]) for i in mine])
        got = run(api, fx, coef, descs, cfg, dest=np.full(coef.size, CANARY, dtype=np.int16))
        signhide, sl = fx["configs"][cfg]
        quant, err = fx["tables"][sl]
        for i in mine:
            c, w, type_, scan, block_type, tr_depth, set_, _ = cs[i]
            want = M.rdoq(c.tolist(), w, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(fx["lambdas"][set_]), fx["dumps"][set_].tolist(), quant, err,
                          signhide)
            assert got[d[i, 0]:d[i, 0] + w * w].tolist() == want, (width, int(i), cs[i][1:])


def test_skipped_descriptors_leave_dest_untouched(api, fx):
    idx = np.concatenate([np.flatnonzero((fx["cfg"] == 0) & (fx["descs"]["width"] == w))[:k] for w, k in ((4, 90), (8, 40), (16, 12), (32, 4))])
    descs = fx["descs"][idx].copy()
    n = fx["coeffs"].size
    want = np.full(n, CANARY, dtype=np.int16)
    m = covered(descs, n)
    want[m] = fx["dest"][m]
    broken = {3: ("width", 12), 10: ("width", 0), 17: ("width", 64), 21: ("type", 1), 30: ("type", 3), 41: ("scan_mode", 3), 50: ("block_type", 0),
              55: ("block_type", 3), 60: ("tr_depth", 4), 64: ("ctx_index", len(fx["sets"])), 77: ("ctx_index", 0xFFFF), 85: ("src_offset", None),
              88: ("dst_offset", None), 95: ("width", 5), 100: ("width", 24), 133: ("type", 4), 140: ("scan_mode", 1), 141: ("scan_mode", 2), 143: ("tr_depth", 255)}
    assert all(descs["width"][i] >= 16 for i in (140, 141))    # a horizontal or vertical scan exists up to width 8 only
    for i, (field, value) in broken.items():
        o, w = int(descs["dst_offset"][i]), int(descs["width"][i])
        want[o:o + w * w] = CANARY
        descs[field][i] = descs[field][i] + 2 if value is None else value
    same(run(api, fx, fx["coeffs"], descs, 0, dest=np.full(n, CANARY, dtype=np.int16)), want, "skipped descriptors")
    # a state whose qp lies outside 0..51 skips its TUs
    states = fx["states"].copy()
    states["qp"][7], states["qp"][9] = -1, 52
    got = run(api, fx, fx["coeffs"], fx["descs"][idx], 0, dest=np.full(n, CANARY, dtype=np.int16), states=states)
    want = np.full(n, CANARY, dtype=np.int16)
    keep = fx["descs"][idx][~np.isin(fx["descs"]["ctx_index"][idx], (7, 9))]
    assert len(keep) < len(idx)
    m = covered(keep, n)
    want[m] = fx["dest"][m]
    same(got, want, "states with a qp outside 0..51")


def test_context_bytes_outside_the_reference_range_and_odd_lambdas_equal_the_model(api, fx):
    """context bytes of 126..255, which the reference's coder never produces, are read as byte & 127 (include/kvz_hip.h), and lambda may be
    any finite positive number: with whole context blocks drawn from 126..255 and lambdas a hundred times too small and too large the
    result is still the model's, byte for byte"""
    idx = np.flatnonzero(fx["cfg"] == 0)[::7]
    g = np.random.default_rng(5)
    dumps = g.integers(126, 256, fx["dumps"].shape).astype(np.uint8)
    lambdas = fx["lambdas"] * np.array((0.01, 1.0, 100.0))[np.arange(len(fx["lambdas"])) % 3]
    sets = np.array([api.coeff_ctx_from_dump(d, 256) for d in dumps], dtype=api.COEFF_CTX)
    states = np.array([api.rdoq_state_from_dump(d, lam, qp) for d, lam, qp in zip(dumps, lambdas, fx["qps"])], dtype=api.RDOQ_STATE)
    assert sets["ctx"][:, :136].min() >= 126 and states["root_cbf"].min() >= 126
    n = fx["coeffs"].size
    got = run(api, fx, fx["coeffs"], fx["descs"][idx], 0, dest=np.full(n, CANARY, dtype=np.int16), sets=sets, states=states)
    quant, err = fx["tables"][0]
    changed = 0
    for i in idx:
        o, w, type_, scan, block_type, tr_depth, set_, _ = fx["d"][i].tolist()
        want = M.rdoq(fx["coeffs"][o:o + w * w].tolist(), w, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(lambdas[set_]), dumps[set_].tolist(),
                      quant, err, 1)
        assert got[o:o + w * w].tolist() == want, (int(i), w, type_, scan, set_)
        changed += int(want != fx["dest"][o:o + w * w].tolist())
    assert changed > len(idx) // 3                              # these inputs decide differently from the recorded ones: the comparison is not idle
    m = covered(fx["descs"][idx], n)
    assert (got[~m] == CANARY).all()


def test_every_error_path_returns_invalid_and_writes_nothing(api, fx):
    from kvazaar_amd import _lib
    L = _lib.load()
    idx = np.flatnonzero(fx["cfg"] == 0)[:40]
    descs = fx["descs"][idx]
    n = fx["coeffs"].size
    quant, err = fx["tables"][0]
    bufs = [api.DeviceBuffer.from_numpy(a) for a in (fx["coeffs"], np.full(n, CANARY, dtype=np.int16), descs, fx["sets"], fx["states"], quant, err)]
    d_c, d_o, d_d, d_s, d_t, d_q, d_e = bufs
    prm = _lib.RdoqParams(1)
    names = ("coef", "dest", "descs", "n", "ctx_sets", "states", "n_sets", "tables", "params")

    def call(quant=d_q.ptr, err_scale=d_e.ptr, **kw):
        tab = _lib.RdoqTables(quant, err_scale)
        a = [d_c.ptr, d_o.ptr, d_d.ptr, len(descs), d_s.ptr, d_t.ptr, len(fx["sets"]), C.pointer(tab), C.pointer(prm), None]
        for k, v in kw.items():
            a[names.index(k)] = v
        return L.kvz_hip_rdoq_batch(*a)

    for broken in (dict(coef=None), dict(dest=None), dict(descs=None), dict(ctx_sets=None), dict(states=None), dict(tables=None), dict(params=None),
                   dict(quant=None), dict(err_scale=None), dict(n_sets=0), dict(n=1 << 31), dict(coef=d_c.ptr + 4), dict(dest=d_o.ptr + 4),
                   dict(descs=d_d.ptr + 2), dict(ctx_sets=d_s.ptr + 1), dict(states=d_t.ptr + 4), dict(quant=d_q.ptr + 8), dict(err_scale=d_e.ptr + 4)):
        assert call(**broken) == -2, broken
        assert b"kvz_hip_rdoq_batch" in L.kvz_hip_last_error()
    assert L.kvz_hip_rdoq_batch(None, None, None, 0, None, None, 0, None, None, None) == 0
    assert (d_o.to_numpy(np.int16, (n,)) == CANARY).all()
    check(api, call(), "rdoq_batch")
    m = covered(descs, n)
    got = d_o.to_numpy(np.int16, (n,))
    same(got[m], fx["dest"][m], "the call with every argument right")
    assert (got[~m] == CANARY).all()


def test_captured_call_replayed_after_the_contents_changed(api, fx):
    from kvazaar_amd import _lib
    L = _lib.load()
    pool = np.flatnonzero(fx["cfg"] == 0)
    rounds = []
    for k in range(2):                                           # two disjoint choices of TUs with the same widths in the same order
        idx = np.concatenate([np.flatnonzero((fx["cfg"] == 0) & (fx["descs"]["width"] == w))[k * c:(k + 1) * c] for w, c in ((4, 120), (8, 80), (16, 30), (32, 6))])
        rounds.append(idx)
    assert len(set(rounds[0]) & set(rounds[1])) == 0 and len(rounds[0]) == len(rounds[1]) and len(pool) > len(rounds[0])
    perm = np.random.default_rng(3).permutation(len(fx["sets"]))         # the second round's records in another order
    contents = []
    for k, idx in enumerate(rounds):
        sizes = fx["descs"]["width"][idx].astype(np.int64) ** 2
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1]))
        coef = np.concatenate([fx["coeffs"][o:o + s] for o, s in zip(fx["descs"]["src_offset"][idx], sizes)])
        want = np.concatenate([fx["dest"][o:o + s] for o, s in zip(fx["descs"]["dst_offset"][idx], sizes)])
        descs = fx["descs"][idx].copy()
        descs["src_offset"] = descs["dst_offset"] = offs
        sets, states = fx["sets"], fx["states"]
        if k == 1:
            sets, states = fx["sets"][perm], fx["states"][perm]
            descs["ctx_index"] = np.argsort(perm)[descs["ctx_index"]]
        contents.append((coef, descs, np.ascontiguousarray(sets), np.ascontiguousarray(states), want))
    assert contents[0][0].size == contents[1][0].size and (contents[0][4] != contents[1][4]).sum() > 1000
    total = contents[0][0].size
    d_c, d_d, d_s, d_t = (api.DeviceBuffer.from_numpy(a) for a in contents[0][:4])
    d_o = api.DeviceBuffer.from_numpy(np.full(total, CANARY, dtype=np.int16))
    quant, err = fx["tables"][0]
    d_q, d_e = api.DeviceBuffer.from_numpy(quant), api.DeviceBuffer.from_numpy(err)
    tab, prm = _lib.RdoqTables(d_q.ptr, d_e.ptr), _lib.RdoqParams(1)
    s, graph = L.kvz_hip_stream_create(), C.c_void_p()
    try:
        check(api, L.kvz_hip_graph_begin(s), "graph_begin")
        check(api, L.kvz_hip_rdoq_batch(d_c.ptr, d_o.ptr, d_d.ptr, len(rounds[0]), d_s.ptr, d_t.ptr, len(fx["sets"]), C.byref(tab), C.byref(prm), s),
              "rdoq_batch (captured)")
        check(api, L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for k, (coef, descs, sets, states, want) in enumerate(contents):
            for buf, a in ((d_c, coef), (d_d, descs), (d_s, sets), (d_t, states)):
                check(api, L.kvz_hip_memcpy_h2d(buf.ptr, a.ctypes.data, a.nbytes, s), "memcpy_h2d")
            check(api, L.kvz_hip_stream_sync(s), "stream_sync")
            check(api, L.kvz_hip_graph_launch(graph, s), "graph_launch")
            check(api, L.kvz_hip_stream_sync(s), "stream_sync")
            same(d_o.to_numpy(np.int16, (total,)), want, "replay %d" % k)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


def test_tus_addressed_as_the_chain_lays_coefficients_out(api, fx):
    """source and destination TUs at LCU * 4096 + the z-order offset of their first 4x4 block, as coeff_y holds them; the result equals
    the contiguous one"""
    layout = [(0, 0, 32), (32, 0, 16), (48, 0, 16), (32, 16, 16), (48, 16, 8), (56, 16, 8), (48, 24, 8), (56, 24, 4), (60, 24, 4), (56, 28, 4), (60, 28, 4),
              (0, 32, 8), (8, 32, 4), (12, 36, 4), (16, 32, 16), (32, 32, 32)]
    by_width = {w: list(np.flatnonzero((fx["cfg"] == 0) & (fx["descs"]["width"] == w) & (fx["descs"]["type"] == 0))) for w in (4, 8, 16, 32)}
    src = np.full(3 * 4096, 77, dtype=np.int16)
    want = np.full(3 * 4096, CANARY, dtype=np.int16)
    rows = []
    for lcu in (0, 2):                                           # the LCU between them stays untouched
        for x, y, n in layout:
            i = by_width[n].pop()
            off = lcu * 4096 + IRC.xy_to_zorder(64, x, y)
            assert off % 16 == 0
            o = int(fx["descs"]["src_offset"][i])
            src[off:off + n * n] = fx["coeffs"][o:o + n * n]
            want[off:off + n * n] = fx["dest"][o:o + n * n]
            dd = fx["descs"][i]
            rows.append((off, off, n, 0, int(dd["scan_mode"]), int(dd["block_type"]), int(dd["tr_depth"]), int(dd["ctx_index"])))
    assert len({r[0] for r in rows}) == len(rows)
    got = run(api, fx, src, make_descs(api, rows), 0, dest=np.full(src.size, CANARY, dtype=np.int16))
    same(got, want, "z-order addressed TUs")

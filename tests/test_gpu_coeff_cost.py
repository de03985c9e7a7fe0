"""GPU: kvz_hip_coeff_cost_batch against tests/golden/coeff_cabac.npz (counts of the compiled reference's own counting coder): the whole
fixture in one call per configuration, byte for byte; the same descriptors cut into calls of 1, 63, 64 and 65 TUs and shuffled; skipped
descriptors; a captured call replayed after the coefficients changed; and descriptors that point into the coeff_y / coeff_u arrays
written by kvz_hip_inter_residual_frame on a 72x72 picture, against the model.  Every test runs under a time limit of its own that ends
the process, and after a call that reports a runtime error no further test starts anything on the device."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

import coeff_cabac_model as M
import inter_residual_cases as IRC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_cabac.npz")
TEST_LIMIT_S = 60                                                     # every test takes a fraction of a second
POISON = 0xDEADBEEF
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


@pytest.fixture(scope="module")
def fx(api):
    """the fixture as the entry takes it: coeffs, descriptors, the sets cut from the dumps, the configuration of every TU, the counts"""
    z = np.load(GOLDEN)
    d = z["desc"].astype(np.int64)
    descs = np.zeros(len(d), dtype=api.COEFF_COST_DESC)
    for k, col in (("offset", 0), ("width", 1), ("type", 2), ("scan_mode", 3), ("tr_skip", 4), ("ctx_index", 5)):
        descs[k] = d[:, col]
    sets = np.array([api.coeff_ctx_from_dump(dump, rng) for dump, rng in zip(z["dumps"], z["ranges"])], dtype=api.COEFF_CTX)
    return dict(coeffs=z["coeffs"], descs=descs, sets=sets, cfg=d[:, 6], configs=[tuple(c) for c in z["configs"].tolist()], bits=z["bits"])


def run(api, fx, descs, cfg, bits=None):
    sh, ts, ll = fx["configs"][cfg]
    try:
        return api.coeff_cost_batch(fx["coeffs"], descs, fx["sets"], sh, ts, ll, bits=bits)
    except Exception:
        FAULTS.append("coeff_cost_batch")
        raise


def same(got, want, what):
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, "%s: %d of %d differ, first at %d: got %d, want %d" % (what, wrong.size, len(want), wrong[0], got[wrong[0]], want[wrong[0]])


def test_whole_fixture_in_one_call_per_configuration(api, fx):
    assert fx["cfg"].tolist().count(0) > len(fx["cfg"]) // 2
    for cfg in range(len(fx["configs"])):
        mine = fx["cfg"] == cfg
        assert mine.sum() >= 4
        got = run(api, fx, fx["descs"], cfg, bits=np.full(len(fx["descs"]), POISON, dtype=np.uint32))      # the WHOLE list each time
        same(got[mine], fx["bits"][mine], "configuration %r" % (fx["configs"][cfg],))
        assert (got != POISON).all()                            # every descriptor is valid: every count was written


@pytest.mark.parametrize("chunk", (1, 63, 64, 65))
def test_cut_into_calls_and_shuffled(api, fx, chunk):
    g = np.random.default_rng(chunk)
    idx = np.flatnonzero(fx["cfg"] == 0)
    idx = g.permutation(idx)[:{1: 24, 63: 63 * 4, 64: 64 * 4, 65: 65 * 4}[chunk]]
    for at in range(0, len(idx), chunk):
        part = idx[at:at + chunk]
        same(run(api, fx, fx["descs"][part], 0), fx["bits"][part], "TUs %d.. in calls of %d" % (at, chunk))


def test_skipped_descriptors_leave_bits_out_untouched(api, fx):
    small = np.flatnonzero(fx["cfg"] == 0)[:150]
    idx = np.concatenate((small, np.flatnonzero((fx["cfg"] == 0) & (fx["descs"]["width"] >= 16))[:10]))
    descs = fx["descs"][idx].copy()
    want = fx["bits"][idx].copy()
    broken = {3: ("width", 12), 10: ("width", 0), 17: ("width", 64), 21: ("type", 1), 30: ("type", 3), 41: ("scan_mode", 3), 55: ("tr_skip", 2),
              64: ("ctx_index", len(fx["sets"])), 77: ("ctx_index", 0xFFFFFFFF), 90: ("offset", None), 127: ("width", 5)}
    for i, (field, value) in broken.items():
        descs[field][i] = descs["offset"][i] + 2 if value is None else value
        want[i] = POISON
    # a horizontal or vertical scan exists up to width 8 only
    wide = [i for i in range(len(descs)) if descs["width"][i] >= 16 and i not in broken][:2]
    assert len(wide) == 2
    for i, mode in zip(wide, (1, 2)):
        descs["scan_mode"][i] = mode
        want[i] = POISON
    same(run(api, fx, descs, 0, bits=np.full(len(descs), POISON, dtype=np.uint32)), want, "skipped descriptors")


def test_context_bytes_outside_the_specified_range_are_harmless(api, fx):
    """the result is specified for bytes 0..125; any other value must still stay inside the tables (nothing to compare, the call completes)"""
    idx = np.flatnonzero(fx["cfg"] == 0)[::9]
    sets = fx["sets"].copy()
    sets["ctx"][:, :] = np.random.default_rng(5).integers(126, 256, sets["ctx"].shape)
    sets["range"][::2] = 0
    sets["range"][1::2] = 65535
    try:
        got = api.coeff_cost_batch(fx["coeffs"], fx["descs"][idx], sets, 1, 1, 0)
    except Exception:
        FAULTS.append("coeff_cost_batch")
        raise
    assert got.shape == (len(idx),)
    same(run(api, fx, fx["descs"][idx], 0), fx["bits"][idx], "the next call")


def test_captured_call_replayed_after_the_coefficients_changed(api, fx):
    from kvazaar_amd import _lib
    L = _lib.load()
    idx = np.concatenate([np.flatnonzero((fx["cfg"] == 0) & (fx["descs"]["width"] == w))[:k] for w, k in ((4, 150), (8, 100), (16, 50))])
    descs = fx["descs"][idx].copy()
    # the TUs packed anew, so that the second contents can be a permutation of the TUs of one size among themselves
    sizes = descs["width"].astype(np.int64) ** 2
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    tus = [fx["coeffs"][o:o + s] for o, s in zip(fx["descs"]["offset"][idx], sizes)]
    descs["offset"] = offs
    first = np.concatenate(tus)
    perm = np.arange(len(idx))
    g = np.random.default_rng(9)
    for w in (4, 8, 16):
        at = np.flatnonzero(descs["width"] == w)
        perm[at] = g.permutation(at)
    second = np.concatenate([tus[j] for j in perm])
    # the count of TU j under the descriptor of slot i: type, scan and set stay the slot's, so the model supplies the second round
    z = np.load(GOLDEN)
    want2 = np.array([M.count_bits(tus[j].tolist(), int(descs["width"][i]), int(descs["type"][i]), int(descs["scan_mode"][i]), int(descs["tr_skip"][i]),
                                   int(z["ranges"][descs["ctx_index"][i]]), z["dumps"][descs["ctx_index"][i]].tolist(), 1, 1, 0)
                      for i, j in enumerate(perm)], dtype=np.uint32)
    assert (want2 != fx["bits"][idx]).sum() > 100
    d_c, d_d, d_s = (api.DeviceBuffer.from_numpy(a) for a in (first, descs, fx["sets"]))
    d_b = api.DeviceBuffer.from_numpy(np.full(len(idx), POISON, dtype=np.uint32))
    prm = _lib.CoeffCostParams(1, 1, 0, 0)
    s, graph = L.kvz_hip_stream_create(), C.c_void_p()
    try:
        check(api, L.kvz_hip_graph_begin(s), "graph_begin")
        check(api, L.kvz_hip_coeff_cost_batch(d_c.ptr, d_d.ptr, len(idx), d_s.ptr, len(fx["sets"]), C.byref(prm), d_b.ptr, s), "coeff_cost_batch (captured)")
        check(api, L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for contents, want, what in ((first, fx["bits"][idx], "first replay"), (second, want2, "replay after the coefficients changed")):
            check(api, L.kvz_hip_memcpy_h2d(d_c.ptr, contents.ctypes.data, contents.nbytes, s), "memcpy_h2d")
            check(api, L.kvz_hip_stream_sync(s), "stream_sync")
            check(api, L.kvz_hip_graph_launch(graph, s), "graph_launch")
            check(api, L.kvz_hip_stream_sync(s), "stream_sync")
            same(d_b.to_numpy(np.uint32, (len(idx),)), want, what)
    finally:
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        L.kvz_hip_stream_destroy(s)


PICTURE = (72, 72, 22, 6)          # width, height, qp, seed: one whole LCU and three ragged ones


def picture_case():
    w, h, qp, seed = PICTURE
    cus, _ = IRC.make_map(w, h, seed, intra_share=0.05, blank_share=0.0)
    pred = IRC.smooth_planes(w, h, seed + 100, 1)
    src = IRC.make_source(pred, cus, seed + 200, 1, amps=(2, 5, 8, 14, 24, 48, 90))
    return src, pred, cus, qp


def picture_descs(api, cus, w, h):
    """one descriptor per TU of the picture's inter CUs, addressed as the chain lays coefficients out: LCU * 4096 (1024) + z-order offset"""
    lcus_x = (w + 63) // 64
    rows = []
    for plane, x, y, n, _, _ in IRC.walk_tus(cus, w, h, 1):
        if plane == 2:
            continue
        lcu = (y // 64) * lcus_x + x // 64
        if plane == 0:
            rows.append((0, lcu * 4096 + IRC.xy_to_zorder(64, x % 64, y % 64), n, 0))
        else:
            rows.append((1, lcu * 1024 + IRC.xy_to_zorder(32, (x % 64) // 2, (y % 64) // 2), n, 2))
    return rows


def test_descriptors_into_the_chains_coefficient_arrays(api):
    src, pred, cus, qp = picture_case()
    w, h = PICTURE[:2]
    try:
        out = api.inter_residual_frame(src, pred, cus, qp, chroma=1, signhide=1)
    except Exception:
        FAULTS.append("inter_residual_frame")
        raise
    rows = picture_descs(api, cus, w, h)
    assert {n for p, _, n, _ in rows if p == 0} == {4, 8, 16, 32} and {n for p, _, n, _ in rows if p == 1} >= {4, 8, 16}
    ranges, dumps = np.random.default_rng(4).integers(256, 511, 4), np.random.default_rng(5).integers(0, 126, (4, 184)).astype(np.uint8)
    sets = np.array([api.coeff_ctx_from_dump(d, r) for d, r in zip(dumps, ranges)], dtype=api.COEFF_CTX)
    lcus_x = (w + 63) // 64
    for plane, type_ in ((0, 0), (1, 2)):
        arr = np.ascontiguousarray(out["coeff"][plane]).ravel()
        mine = [r for r in rows if r[0] == plane]
        descs = np.zeros(len(mine), dtype=api.COEFF_COST_DESC)
        want = np.zeros(len(mine), dtype=np.uint32)
        for i, (_, off, n, t) in enumerate(mine):
            set_ = (off // (4096 if plane == 0 else 1024)) % 4     # a set per LCU, as a search would use them
            descs[i] = (off, n, t, 0, 0, set_)
            want[i] = M.count_bits(arr[off:off + n * n].tolist(), n, t, 0, 0, int(ranges[set_]), dumps[set_].tolist(), 1, 1, 0)
        assert (want > 0).sum() > len(want) // 3 and (want == 0).any()
        try:
            got = api.coeff_cost_batch(arr, descs, sets, 1, 1, 0, bits=np.full(len(descs), POISON, dtype=np.uint32))
        except Exception:
            FAULTS.append("coeff_cost_batch")
            raise
        same(got, want, "plane %d" % plane)
    assert lcus_x == 2

"""GPU: the three headline kernels at the edges of their launch geometry, bit for bit against the oracle.

  * sad / satd at 8x8 (and the sad dual entry) store their results with the nontemporal policy ("cost_store_nt" 1, the default)
    or the default one (0); 16x16 has the same kernel shape and one store.  A wave iteration is 64 blocks at 8x8 and 16 at 16x16, a workgroup four of them: the
    counts sit on and around those edges, and one launch with a single workgroup per CU makes every wave loop and ends ragged.
  * dct_32x32 with one block per wave (the default grid) at counts around a workgroup's four blocks, with the extremes of int16,
    and with a capped grid whose waves take several blocks.
Every output array is followed by 64 sentinel words that must stay as they were.  Every knob is restored to its default (-1)
whatever happens."""
import numpy as np
import pytest

import oracle_lib as O
from patterns import rng

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
COUNTS8 = (1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4099)
COUNTS16 = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000)
COUNTS32 = (1, 2, 3, 4, 5, 7, 8, 9, 1023)
LOOP8, LOOP32 = 70000, 3000          # more than one sweep of a grid of one workgroup per CU (256 CUs: 65 536 blocks / 1024 blocks)


@pytest.fixture(scope="module")
def env():
    from kvazaar_amd import _lib, api
    return api, _lib, _lib.init(0)


@pytest.fixture
def knobs(env):
    """knobs(key=value, ...) sets tuning knobs; every knob set is back at its default after the test"""
    with env[0].tuned() as set_:
        yield set_


def block_pairs(n, count, seed):
    """random pairs a few levels apart, with the extremes mixed in: equal blocks, 255 against 0, a checkerboard"""
    g = rng(seed)
    a = g.integers(0, 256, (count, n * n), dtype=np.uint8)
    b = np.clip(a.astype(np.int32) + g.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    b[1::5] = a[1::5]
    a[2::7], b[2::7] = 255, 0
    a[3::11, ::2], b[3::11, ::2] = 0, 255
    return a, b


@pytest.fixture(scope="module")
def pools():
    """{(kind, n): (blk1, blk2, costs of the oracle)}: one pool per kernel, every count is a prefix of it"""
    out = {}
    for n, most in ((8, LOOP8), (16, max(COUNTS16))):
        a, b = block_pairs(n, most, 80 + n)
        for kind in ("sad", "satd"):
            want = O.cost_nxn_batch(kind, n, a, b)
            want.setflags(write=False)
            out[kind, n] = (a, b, want)
    return out


def guarded(api, words):
    """a device array of `words` 32-bit words followed by 64 sentinel words; the words themselves start as the sentinel's complement"""
    host = np.full(words + 64, SENTINEL, dtype=np.uint32)
    host[:words] = ~np.uint32(SENTINEL)
    return api.DeviceBuffer.from_numpy(host)


def read_guarded(buf, words, tag):
    got = buf.to_numpy(np.uint32, (words + 64,))
    assert (got[words:] == SENTINEL).all(), "words behind the output were written: %s" % tag
    return got[:words]


def run_cost(env, kind, n, a, b, count):
    api, _lib, L = env
    da, db, out = api.DeviceBuffer.from_numpy(a[:count]), api.DeviceBuffer.from_numpy(b[:count]), guarded(api, count)
    f = L.kvz_hip_sad_nxn_batch if kind == "sad" else L.kvz_hip_satd_nxn_batch
    _lib.check(f(n, da.ptr, db.ptr, count, out.ptr, None), "%s_%dx%d" % (kind, n, n))
    return read_guarded(out, count, "%s_%dx%d count=%d" % (kind, n, n, count))


@pytest.mark.parametrize("n,counts,nt", ((8, COUNTS8, 1), (8, COUNTS8, 0), (16, COUNTS16, 1)))
@pytest.mark.parametrize("kind", ("sad", "satd"))
def test_cost_counts(env, knobs, pools, kind, n, counts, nt):
    knobs(cost_store_nt=nt)
    a, b, want = pools[kind, n]
    for count in counts:
        got = run_cost(env, kind, n, a, b, count)
        np.testing.assert_array_equal(got, want[:count], err_msg="%s_%dx%d count=%d cost_store_nt=%d" % (kind, n, n, count, nt))


@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("kind", ("sad", "satd"))
def test_cost8_waves_loop(env, knobs, pools, kind, nt):
    """one workgroup per CU and 70 000 blocks: every wave takes a second iteration, the last one is ragged"""
    knobs(cost_store_nt=nt, sad_wgs_per_cu=1, satd8_wgs_per_cu=1)
    a, b, want = pools[kind, 8]
    got = run_cost(env, kind, 8, a, b, LOOP8)
    np.testing.assert_array_equal(got, want, err_msg="%s_8x8 count=%d one workgroup per CU cost_store_nt=%d" % (kind, LOOP8, nt))


@pytest.mark.parametrize("n,nt", ((8, 1), (8, 0), (16, 1)))
def test_sad_dual(env, knobs, n, nt):
    """sad_NxN_dual: two predictions per item inside a strided array, the same kernel template with two results per item"""
    api, _lib, L = env
    knobs(cost_store_nt=nt)
    ps, its = 1024, 2048
    for items in (1, 3, 33):
        g = rng(900 + 10 * n + items)
        orig = g.integers(0, 256, (items, n * n), dtype=np.uint8)
        preds = g.integers(0, 256, (items, its), dtype=np.uint8)
        preds[:, :n * n] = np.clip(orig.astype(np.int32) + g.integers(-9, 10, orig.shape), 0, 255)
        want = O.cost_nxn_dual_batch("sad", n, preds, orig, ps)
        dp, do, out = api.DeviceBuffer.from_numpy(preds), api.DeviceBuffer.from_numpy(orig), guarded(api, 2 * items)
        _lib.check(L.kvz_hip_sad_nxn_dual_batch(n, dp.ptr, ps, its, do.ptr, items, out.ptr, None), "sad_%dx%d_dual" % (n, n))
        tag = "sad_%dx%d_dual items=%d cost_store_nt=%d" % (n, n, items, nt)
        np.testing.assert_array_equal(read_guarded(out, 2 * items, tag).reshape(items, 2), want, err_msg=tag)


@pytest.fixture(scope="module")
def residuals():
    """{name: (blocks, coefficients of the oracle)}: random in +-255 (LOOP32 blocks, the counts are prefixes) and the two extremes"""
    out = {}
    for name, x in (("random", rng(3232).integers(-255, 256, (LOOP32, 1024)).astype(np.int16)),
                    ("max", np.full((max(COUNTS32), 1024), 32767, dtype=np.int16)),
                    ("min", np.full((max(COUNTS32), 1024), -32768, dtype=np.int16))):
        # the extremes are the same block over and over: one oracle call
        want = O.transform_batch("dct", 32, x) if name == "random" else np.repeat(O.transform_batch("dct", 32, x[:1]), x.shape[0], axis=0)
        want.setflags(write=False)
        out[name] = (x, want)
    return out


def run_dct32(env, x, count):
    api, _lib, L = env
    words = count * 512                                   # 1024 int16 per block
    dx, out = api.DeviceBuffer.from_numpy(x[:count]), guarded(api, words)
    _lib.check(L.kvz_hip_transform_batch(api.KINDS["dct"], 32, dx.ptr, out.ptr, count, None), "dct_32x32")
    return read_guarded(out, words, "dct_32x32 count=%d" % count).view(np.int16).reshape(count, 1024)


@pytest.mark.parametrize("data", ("random", "max", "min"))
def test_dct32_counts(env, residuals, data):
    x, want = residuals[data]
    for count in COUNTS32:
        np.testing.assert_array_equal(run_dct32(env, x, count), want[:count], err_msg="dct_32x32 %s count=%d" % (data, count))


def test_dct32_capped_grid_loops(env, knobs, residuals):
    """one workgroup per CU and 3000 blocks: every wave takes a second and a third block, the last sweep is ragged"""
    knobs(dct32_wgs_per_cu=1)
    x, want = residuals["random"]
    np.testing.assert_array_equal(run_dct32(env, x, LOOP32), want, err_msg="dct_32x32 count=%d one workgroup per CU" % LOOP32)

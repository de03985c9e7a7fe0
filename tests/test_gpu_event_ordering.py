"""Events of the C ABI under every `event_fence` setting (kvz_hip_set_tuning; 0 = no system fence, 1 = release to the device,
2 = HIP's default event): they still time device work, still order one stream of a device behind another, and
kvz_hip_stream_sync is what publishes results to the host (include/kvz_hip.h states the contract)."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
from patterns import rng

pytestmark = pytest.mark.gpu

FENCES = (0, 1, 2)
PAIRS = 1024                    # 64 KiB of 8x8 blocks
ROUNDS = 16


@pytest.fixture(scope="module")
def L():
    from kvazaar_amd import _lib
    return _lib.init(0)


@pytest.fixture
def fence(L, request):
    """events created inside the test take the flag of this setting; the library's default comes back afterwards"""
    from kvazaar_amd import _lib
    _lib.check(L.kvz_hip_set_tuning(b"event_fence", request.param), "set_tuning")
    yield request.param
    _lib.check(L.kvz_hip_set_tuning(b"event_fence", -1), "set_tuning")


@pytest.fixture(scope="module")
def patterns():
    """ROUNDS current-block patterns, the fixed reference blocks and the oracle's costs of every round (computed once)"""
    g = rng(9100)
    fixed = g.integers(0, 256, (PAIRS, 64), dtype=np.uint8)
    pats = g.integers(0, 256, (ROUNDS, PAIRS, 64), dtype=np.uint8)
    want = np.stack([O.cost_nxn_many("sad", 8, pats[k], fixed) for k in range(ROUNDS)])
    assert all((want[k] != want[k - 1]).any() for k in range(1, ROUNDS))      # a stale read cannot pass for a fresh one
    return fixed, pats, want


def _elapsed(L, a, b):
    from kvazaar_amd import _lib
    f = C.c_float()
    _lib.check(L.kvz_hip_event_elapsed_ms(a, b, C.byref(f)), "event_elapsed")
    return f.value


@pytest.mark.parametrize("fence", FENCES, indirect=True)
def test_events_time_a_launch(L, fence):
    from kvazaar_amd import _lib
    from kvazaar_amd.api import DeviceBuffer
    g = rng(9000 + fence)
    n = 4096
    a = DeviceBuffer.from_numpy(g.integers(0, 256, (n, 64), dtype=np.uint8))
    b = DeviceBuffer.from_numpy(g.integers(0, 256, (n, 64), dtype=np.uint8))
    out = DeviceBuffer(4 * n)
    s = L.kvz_hip_stream_create()
    ev = [L.kvz_hip_event_create() for _ in range(4)]
    assert all(ev)
    try:
        _lib.check(L.kvz_hip_sad_nxn_batch(8, a.ptr, b.ptr, n, out.ptr, s), "sad")          # code object loaded before the brackets
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        # three brackets of each kind; the smallest of each is compared, so that a pause of the host thread between two
        # of the calls below cannot decide the test
        with_launch, empty = [], []
        for _ in range(3):
            _lib.check(L.kvz_hip_event_record(ev[0], s), "record")
            _lib.check(L.kvz_hip_sad_nxn_batch(8, a.ptr, b.ptr, n, out.ptr, s), "sad")
            _lib.check(L.kvz_hip_event_record(ev[1], s), "record")
            _lib.check(L.kvz_hip_event_record(ev[2], s), "record")
            _lib.check(L.kvz_hip_event_record(ev[3], s), "record")
            with_launch.append(_elapsed(L, ev[0], ev[1]))
            empty.append(_elapsed(L, ev[2], ev[3]))
        print("event_fence %d: bracket with a launch %s ms, empty bracket %s ms" % (fence, with_launch, empty))
        for ms in with_launch:
            assert math.isfinite(ms) and ms > 0
        for ms in empty:
            assert math.isfinite(ms) and ms >= 0
        assert min(with_launch) >= min(empty)
    finally:
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        for e in ev:
            L.kvz_hip_event_destroy(e)
        L.kvz_hip_stream_destroy(s)


def _rounds(L, patterns, read_back):
    """ROUNDS times: stream A copies pattern k into the shared buffer and records an event, stream B waits for it and scores the
    buffer against the fixed blocks into the costs of round k.  A second event keeps A's next copy behind B's read."""
    from kvazaar_amd import _lib
    from kvazaar_amd.api import DeviceBuffer
    fixed, pats, want = patterns
    d_fixed, d_pats = DeviceBuffer.from_numpy(fixed), DeviceBuffer.from_numpy(pats)
    d_buf, d_cost = DeviceBuffer(PAIRS * 64), DeviceBuffer(4 * PAIRS * ROUNDS)
    sa, sb = L.kvz_hip_stream_create(), L.kvz_hip_stream_create()
    filled, scored = L.kvz_hip_event_create(), L.kvz_hip_event_create()
    assert filled and scored
    try:
        _lib.check(L.kvz_hip_memset(d_cost.ptr, 0xFF, d_cost.nbytes, sb), "memset")
        for k in range(ROUNDS):
            _lib.check(L.kvz_hip_memcpy_d2d(d_buf.ptr, d_pats.ptr + k * PAIRS * 64, PAIRS * 64, sa), "fill")
            _lib.check(L.kvz_hip_event_record(filled, sa), "record filled")
            _lib.check(L.kvz_hip_stream_wait_event(sb, filled), "wait filled")
            _lib.check(L.kvz_hip_sad_nxn_batch(8, d_buf.ptr, d_fixed.ptr, PAIRS, d_cost.ptr + 4 * PAIRS * k, sb), "sad")
            _lib.check(L.kvz_hip_event_record(scored, sb), "record scored")
            _lib.check(L.kvz_hip_stream_wait_event(sa, scored), "wait scored")
        return read_back(d_cost, sa, sb)
    finally:
        _lib.check(L.kvz_hip_stream_sync(sa), "sync")
        _lib.check(L.kvz_hip_stream_sync(sb), "sync")
        L.kvz_hip_event_destroy(filled); L.kvz_hip_event_destroy(scored)
        L.kvz_hip_stream_destroy(sa); L.kvz_hip_stream_destroy(sb)


@pytest.mark.parametrize("fence", FENCES, indirect=True)
def test_event_orders_a_second_stream(L, fence, patterns):
    got = _rounds(L, patterns, lambda d_cost, sa, sb: d_cost.to_numpy(np.uint32, (ROUNDS, PAIRS), stream=sb))
    for k in range(ROUNDS):
        np.testing.assert_array_equal(got[k], patterns[2][k], err_msg="event_fence %d, round %d" % (fence, k))


@pytest.mark.parametrize("fence", FENCES, indirect=True)
def test_stream_sync_publishes_to_the_host(L, fence, patterns):
    from kvazaar_amd import _lib

    def read_back(d_cost, sa, sb):
        _lib.check(L.kvz_hip_stream_sync(sb), "sync")
        side = L.kvz_hip_stream_create()                 # not the stream the costs were written on
        try:
            return d_cost.to_numpy(np.uint32, (ROUNDS, PAIRS), stream=side)
        finally:
            L.kvz_hip_stream_destroy(side)
    got = _rounds(L, patterns, read_back)
    np.testing.assert_array_equal(got, patterns[2], err_msg="event_fence %d" % fence)

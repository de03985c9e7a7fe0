"""Event records that ride on the launch in front of them (tuning key `event_alias`, kvazaar_amd/csrc/event_alias.h and api.hip): with
the key on and off, under the event flavours of `event_fence`, the ABI's events still time launches, still order a second stream, stop
standing for a launch as soon as anything else is enqueued behind it, stay real records inside a capture, and come and go by the
hundreds.  What the launches compute is the oracle's in every setting."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
from patterns import rng

pytestmark = pytest.mark.gpu

PAIRS = 65536                   # 8x8 pairs of the timed sequence: 4 MiB per operand, a launch of microseconds
BLOCKS = 256                    # 32x32 residual blocks of the timed sequence
ROUNDS = 16
ROUND_PAIRS = 262144            # pairs per round of the ordering test: the producer runs for tens of microseconds
SETTINGS = [(alias, fence) for alias in (0, 1) for fence in (0, 2)]


@pytest.fixture(scope="module")
def L():
    from kvazaar_amd import _lib
    return _lib.init(0)


@pytest.fixture
def setting(L, request):
    """(event_alias, event_fence) for the test's records, launches and events; the library's defaults come back afterwards"""
    from kvazaar_amd import _lib
    alias, fence = request.param
    _lib.check(L.kvz_hip_set_tuning(b"event_alias", alias), "set_tuning")
    _lib.check(L.kvz_hip_set_tuning(b"event_fence", fence), "set_tuning")
    yield request.param
    _lib.check(L.kvz_hip_set_tuning(b"event_alias", -1), "set_tuning")
    _lib.check(L.kvz_hip_set_tuning(b"event_fence", -1), "set_tuning")


@pytest.fixture(scope="module")
def step_data():
    """inputs of one sad_8x8 + satd_8x8 + dct_32x32 step and the oracle's results (computed once, never written)"""
    g = rng(9200)
    cur = g.integers(0, 256, (PAIRS, 64), dtype=np.uint8)
    ref = np.clip(cur.astype(np.int16) + g.integers(-8, 9, cur.shape), 0, 255).astype(np.uint8)
    res = g.integers(-255, 256, (BLOCKS, 1024)).astype(np.int16)
    want = (O.cost_nxn_many("sad", 8, cur, ref), O.cost_nxn_many("satd", 8, cur, ref), O.transform_many("dct", 32, res))
    return cur, ref, res, want


@pytest.fixture(scope="module")
def round_data():
    """round k scores blocks k .. k + ROUND_PAIRS of one array against fixed blocks: ROUNDS different cost vectors from 16 MiB"""
    g = rng(9201)
    base = g.integers(0, 256, (ROUND_PAIRS + ROUNDS, 64), dtype=np.uint8)
    fixed = g.integers(0, 256, (ROUND_PAIRS, 64), dtype=np.uint8)
    want = np.stack([O.cost_nxn_many("sad", 8, base[k:k + ROUND_PAIRS], fixed) for k in range(ROUNDS)])
    assert all((want[k] != want[k - 1]).any() for k in range(1, ROUNDS))      # a stale read cannot pass for a fresh one
    return base, fixed, want


def _elapsed(L, a, b):
    from kvazaar_amd import _lib
    f = C.c_float()
    _lib.check(L.kvz_hip_event_elapsed_ms(a, b, C.byref(f)), "event_elapsed")
    return f.value


class Step:
    """device buffers of step_data and the bracketed sequence record e0; sad; record e1; satd; record e2; dct; record e3; record e4"""

    def __init__(self, L, step_data):
        from kvazaar_amd.api import DeviceBuffer
        cur, ref, res, _ = step_data
        self.L = L
        self.cur, self.ref, self.res = DeviceBuffer.from_numpy(cur), DeviceBuffer.from_numpy(ref), DeviceBuffer.from_numpy(res)
        self.sad, self.satd, self.coef = DeviceBuffer(4 * PAIRS), DeviceBuffer(4 * PAIRS), DeviceBuffer(res.nbytes)

    def poison(self, s):
        from kvazaar_amd import _lib
        for b in (self.sad, self.satd, self.coef):
            _lib.check(self.L.kvz_hip_memset(b.ptr, 0xFF, b.nbytes, s), "memset")

    def launch_sad(self, s):
        from kvazaar_amd import _lib
        _lib.check(self.L.kvz_hip_sad_nxn_batch(8, self.cur.ptr, self.ref.ptr, PAIRS, self.sad.ptr, s), "sad_8x8")

    def launch_satd(self, s):
        from kvazaar_amd import _lib
        _lib.check(self.L.kvz_hip_satd_nxn_batch(8, self.cur.ptr, self.ref.ptr, PAIRS, self.satd.ptr, s), "satd_8x8")

    def launch_dct(self, s):
        from kvazaar_amd import _lib
        _lib.check(self.L.kvz_hip_transform_batch(0, 32, self.res.ptr, self.coef.ptr, BLOCKS, s), "dct_32x32")

    def bracketed(self, s, ev):
        from kvazaar_amd import _lib
        L = self.L
        _lib.check(L.kvz_hip_event_record(ev[0], s), "record")
        for i, launch in enumerate((self.launch_sad, self.launch_satd, self.launch_dct)):
            launch(s)
            _lib.check(L.kvz_hip_event_record(ev[i + 1], s), "record")
        _lib.check(L.kvz_hip_event_record(ev[4], s), "record")

    def results(self, s):
        return (self.sad.to_numpy(np.uint32, (PAIRS,), stream=s), self.satd.to_numpy(np.uint32, (PAIRS,), stream=s),
                self.coef.to_numpy(np.int16, (BLOCKS, 1024), stream=s))


def _check_brackets(L, ev, what):
    parts = [_elapsed(L, ev[i], ev[i + 1]) for i in range(3)]
    whole, empty = _elapsed(L, ev[0], ev[3]), _elapsed(L, ev[3], ev[4])
    for ms in parts + [whole]:
        assert math.isfinite(ms) and ms > 0, (what, parts, whole)
    assert math.isfinite(empty) and empty >= 0, (what, empty)
    return parts, whole, empty


_outputs = {}                   # fence -> {alias: the three result arrays}: the two settings of event_alias compute the same bytes


@pytest.mark.parametrize("setting", SETTINGS, indirect=True)
def test_times_add_up(L, setting, step_data):
    from kvazaar_amd import _lib
    alias, fence = setting
    st = Step(L, step_data)
    s = L.kvz_hip_stream_create()
    ev = [L.kvz_hip_event_create() for _ in range(5)]
    assert s and all(ev)
    try:
        st.bracketed(s, ev)                             # code objects loaded before the brackets that count
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        st.poison(s)
        st.bracketed(s, ev)
        parts, whole, empty = _check_brackets(L, ev, setting)
        print("event_alias %d event_fence %d: sad %.5f satd %.5f dct %.5f sum %.5f whole %.5f empty %.5f ms"
              % (alias, fence, parts[0], parts[1], parts[2], sum(parts), whole, empty))
        # differences of nanosecond end stamps of one clock, returned as float milliseconds: rounding only
        assert abs(sum(parts) - whole) <= 1e-3
        # what shows that the records really rode on the launches: e3 and e4 then stand for one instant, the end of dct_32x32, and the
        # time between them is exactly 0; two marker packets are two instants, a packet's own time apart
        if alias:
            assert empty == 0.0, "event_alias 1: the records behind dct_32x32 were packets of their own (%.5f ms apart)" % empty
        else:
            assert empty > 0.0, "event_alias 0: two records share an instant"
        got = st.results(s)
        for g, w, name in zip(got, step_data[3], ("sad_8x8", "satd_8x8", "dct_32x32")):
            np.testing.assert_array_equal(g, w, err_msg="%s, event_alias %d event_fence %d" % (name, alias, fence))
        _outputs.setdefault(fence, {})[alias] = got
        both = _outputs[fence]
        if len(both) == 2:
            for a, b in zip(both[0], both[1]):
                assert a.tobytes() == b.tobytes()
    finally:
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        for e in ev:
            L.kvz_hip_event_destroy(e)
        L.kvz_hip_stream_destroy(s)


@pytest.mark.parametrize("setting", SETTINGS, indirect=True)
def test_an_aliased_event_orders_a_second_stream(L, setting, round_data):
    """ROUNDS times: stream A records, scores pattern k into the cost buffer and records `filled`; stream B waits for it and copies the
    buffer into slot k; a second event keeps A's next launch behind B's copy"""
    from kvazaar_amd import _lib
    from kvazaar_amd.api import DeviceBuffer
    base, fixed, want = round_data
    d_base, d_fixed = DeviceBuffer.from_numpy(base), DeviceBuffer.from_numpy(fixed)
    d_cost, d_slots = DeviceBuffer(4 * ROUND_PAIRS), DeviceBuffer(4 * ROUND_PAIRS * ROUNDS)
    sa, sb = L.kvz_hip_stream_create(), L.kvz_hip_stream_create()
    before, filled, done = (L.kvz_hip_event_create() for _ in range(3))
    assert sa and sb and before and filled and done
    try:
        _lib.check(L.kvz_hip_memset(d_cost.ptr, 0xFF, d_cost.nbytes, sa), "memset")
        _lib.check(L.kvz_hip_memset(d_slots.ptr, 0xFF, d_slots.nbytes, sb), "memset")
        for k in range(ROUNDS):
            _lib.check(L.kvz_hip_event_record(before, sa), "record before")
            _lib.check(L.kvz_hip_sad_nxn_batch(8, d_base.ptr + 64 * k, d_fixed.ptr, ROUND_PAIRS, d_cost.ptr, sa), "sad")
            _lib.check(L.kvz_hip_event_record(filled, sa), "record filled")
            _lib.check(L.kvz_hip_stream_wait_event(sb, filled), "wait filled")
            _lib.check(L.kvz_hip_memcpy_d2d(d_slots.ptr + 4 * ROUND_PAIRS * k, d_cost.ptr, 4 * ROUND_PAIRS, sb), "copy")
            _lib.check(L.kvz_hip_event_record(done, sb), "record done")
            _lib.check(L.kvz_hip_stream_wait_event(sa, done), "wait done")
        _lib.check(L.kvz_hip_stream_sync(sa), "sync")
        got = d_slots.to_numpy(np.uint32, (ROUNDS, ROUND_PAIRS), stream=sb)
        for k in range(ROUNDS):
            np.testing.assert_array_equal(got[k], want[k], err_msg="event_alias %d event_fence %d, round %d" % (setting + (k,)))
    finally:
        _lib.check(L.kvz_hip_stream_sync(sa), "sync")
        _lib.check(L.kvz_hip_stream_sync(sb), "sync")
        for e in (before, filled, done):
            L.kvz_hip_event_destroy(e)
        L.kvz_hip_stream_destroy(sa); L.kvz_hip_stream_destroy(sb)


@pytest.mark.parametrize("setting", [(0, 0), (1, 0)], indirect=True)
def test_an_operation_in_between_ends_the_alias(L, setting, step_data):
    from kvazaar_amd import _lib
    from kvazaar_amd.api import DeviceBuffer
    big, tail = 64 << 20, 4096
    st = Step(L, step_data)
    d_big, d_tail = DeviceBuffer(big), DeviceBuffer(tail)
    sa, sb = L.kvz_hip_stream_create(), L.kvz_hip_stream_create()
    before, ev = L.kvz_hip_event_create(), L.kvz_hip_event_create()
    assert sa and sb and before and ev
    try:
        _lib.check(L.kvz_hip_memset(d_big.ptr, 0x11, big, sa), "memset")
        _lib.check(L.kvz_hip_memset(d_tail.ptr, 0x22, tail, sa), "memset")
        _lib.check(L.kvz_hip_stream_sync(sa), "sync")
        _lib.check(L.kvz_hip_event_record(before, sa), "record")
        st.launch_sad(sa)
        _lib.check(L.kvz_hip_memset(d_big.ptr, 0x5A, big, sa), "memset")
        _lib.check(L.kvz_hip_event_record(ev, sa), "record")
        _lib.check(L.kvz_hip_stream_wait_event(sb, ev), "wait")
        _lib.check(L.kvz_hip_memcpy_d2d(d_tail.ptr, d_big.ptr + big - tail, tail, sb), "copy")
        got = d_tail.to_numpy(np.uint8, (tail,), stream=sb)
        assert (got == 0x5A).all(), "event_alias %d: %d of %d bytes read before the memset" % (setting[0], int((got != 0x5A).sum()), tail)
    finally:
        _lib.check(L.kvz_hip_stream_sync(sa), "sync")
        _lib.check(L.kvz_hip_stream_sync(sb), "sync")
        L.kvz_hip_event_destroy(before); L.kvz_hip_event_destroy(ev)
        L.kvz_hip_stream_destroy(sa); L.kvz_hip_stream_destroy(sb)


@pytest.mark.parametrize("setting", [(0, 0), (1, 0)], indirect=True)
def test_records_inside_a_capture_stay_records(L, setting, step_data):
    """record; sad_8x8; record on the captured stream, satd_8x8 on a stream forked off and joined back by record / wait pairs"""
    from kvazaar_amd import _lib
    st = Step(L, step_data)
    s, side = L.kvz_hip_stream_create(), L.kvz_hip_stream_create()
    fork, join, e0, e1 = (L.kvz_hip_event_create() for _ in range(4))
    graph = C.c_void_p()
    assert s and side and fork and join and e0 and e1
    try:
        st.launch_sad(s); st.launch_satd(s)             # code objects loaded before the capture
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        _lib.check(L.kvz_hip_graph_begin(s), "graph_begin")
        _lib.check(L.kvz_hip_event_record(fork, s), "fork")
        _lib.check(L.kvz_hip_stream_wait_event(side, fork), "fork wait")
        st.launch_satd(side)
        _lib.check(L.kvz_hip_event_record(e0, s), "record")
        st.launch_sad(s)
        _lib.check(L.kvz_hip_event_record(e1, s), "record")
        _lib.check(L.kvz_hip_event_record(join, side), "join record")
        _lib.check(L.kvz_hip_stream_wait_event(s, join), "join wait")
        _lib.check(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
        assert graph.value
        for replay in range(2):
            st.poison(s)
            _lib.check(L.kvz_hip_graph_launch(graph, s), "graph_launch")
            sad, satd, _ = st.results(s)
            np.testing.assert_array_equal(sad, step_data[3][0], err_msg="sad_8x8, replay %d, event_alias %d" % (replay, setting[0]))
            np.testing.assert_array_equal(satd, step_data[3][1], err_msg="satd_8x8, replay %d, event_alias %d" % (replay, setting[0]))
    finally:
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        _lib.check(L.kvz_hip_stream_sync(side), "sync")
        if graph.value:
            L.kvz_hip_graph_destroy(graph)
        for e in (fork, join, e0, e1):
            L.kvz_hip_event_destroy(e)
        L.kvz_hip_stream_destroy(s); L.kvz_hip_stream_destroy(side)


@pytest.mark.parametrize("setting", [(0, 0), (1, 0)], indirect=True)
def test_many_events(L, setting, step_data):
    """200 steps with fresh events each, as bench.py keeps them; every time is read afterwards"""
    from kvazaar_amd import _lib
    st = Step(L, step_data)
    s = L.kvz_hip_stream_create()
    evs = [[L.kvz_hip_event_create() for _ in range(5)] for _ in range(200)]
    assert s and all(all(ev) for ev in evs)
    try:
        st.launch_sad(s); st.launch_satd(s); st.launch_dct(s)
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        for ev in evs:
            st.bracketed(s, ev)
        for k, ev in enumerate(evs):
            _, _, empty = _check_brackets(L, ev, (setting, k))
            if setting[0]:
                assert empty == 0.0, (k, empty)         # aliased in every step, the 200th like the first
        for a, b in zip(evs, evs[1:]):                  # and from one step to the next
            ms = _elapsed(L, a[4], b[0])
            assert math.isfinite(ms) and ms >= 0
    finally:
        _lib.check(L.kvz_hip_stream_sync(s), "sync")
        for ev in evs:
            for e in ev:
                L.kvz_hip_event_destroy(e)
        L.kvz_hip_stream_destroy(s)
        _lib.check(L.kvz_hip_stream_sync(None), "sync")

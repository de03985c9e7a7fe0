"""GPU: the sub-pel sample kernels and the fractional search on every dispatch branch, bit for bit against the oracle.

  * the chunked path of the workgroup-per-block kernels: "wg_chunk_min_wgs" at its default over lists of at least 16384
    descriptors (chunk >= 4), at 0 (chunk 1) and at 1 (chunk 64), on lists where every 64-slot window mixes the size classes,
    some windows hold more than 32 big blocks above slot 32, consecutive big blocks alternate shape and interior / clamped
    windows, and the ragged last workgroup holds a big block;
  * "sample8_wave" 0 and 1 (8x8 luma on the general path and on the one-wave path);
  * a plane whose row stride exceeds ref_w, with padding unlike the edge pixels, outputs placed out of list order at odd
    offsets with canaries between them, unsupported descriptors that must leave their bytes untouched;
  * one motion-compensation pass and one fractional search pass of a 1920x1080 frame at the default knobs;
  * malformed fractional search descriptors flagged by the big kernel between well-formed ones;
  * "intra_rough_waves" 4 and 8 at every PU size.
Every knob is restored to its default (-1) whatever happens."""
import numpy as np
import pytest

import oracle_lib as O
from patterns import intra_ref_cases, rng

pytestmark = pytest.mark.gpu

KINDS = ("luma", "luma14", "chroma", "chroma14")
CHUNK_COUNT = 16384 + 37            # chunk 4 at the default knob (last workgroup: 1 slot), 64 at knob 1 (last: 37 slots)
PAD = 200                           # edge padding of the oracle's planes: every window of the tests lies inside it
CANARY = 0xA5                       # byte pattern of every output buffer before a launch
FLAG_FILL = 0x5A5A5A5A              # fractional search outputs before a launch (the flag value is 0xFFFFFFFF)

LUMA_BIG = ((64, 64), (32, 32), (64, 32), (32, 64), (64, 16), (16, 64), (64, 48), (48, 64), (32, 8), (8, 32), (32, 24), (24, 32),
            (32, 16), (16, 32), (17, 3), (64, 5), (21, 40), (36, 17), (63, 63), (48, 24))
LUMA_SMALL = ((8, 8), (16, 16), (8, 4), (4, 8), (16, 4), (4, 16), (16, 12), (12, 16), (16, 8), (8, 16), (8, 8), (5, 3), (1, 1),
              (6, 6), (12, 7), (16, 2))
CHROMA_BIG = ((32, 32), (32, 16), (16, 32), (32, 8), (8, 32), (32, 24), (24, 32), (31, 32), (17, 3), (20, 17), (32, 5), (32, 4))
CHROMA_SMALL = ((4, 4), (8, 8), (4, 2), (2, 4), (8, 2), (2, 8), (6, 8), (8, 6), (16, 16), (8, 4), (1, 1), (3, 5), (16, 12), (2, 2))
FRAC_SMALL = ((8, 8), (16, 16), (8, 4), (4, 8), (16, 4), (4, 16), (16, 12), (12, 16), (16, 8), (8, 16), (4, 12), (12, 8))
FRAC_MEDIUM = ((32, 32), (32, 8), (8, 32), (32, 16), (16, 32), (32, 24), (24, 32), (24, 8), (20, 32), (32, 28))
FRAC_BIG = ((64, 64), (64, 32), (32, 64), (64, 16), (16, 64), (64, 48), (48, 64), (64, 8), (40, 64), (64, 36))
FRAC_MALFORMED = ((12, 12), (4, 4), (6, 8), (68, 8), (8, 0), (-4, 8))


@pytest.fixture(scope="module")
def env():
    from kvazaar_amd import _lib, api
    return api, _lib, _lib.init(0)


@pytest.fixture
def knobs(env):
    """knobs(key=value, ...) sets tuning knobs; every knob set is back at its default after the test"""
    with env[0].tuned() as set_:
        yield set_


# ------------------------------------------------------------------ planes
def frame_of(h, w, seed):
    """a frame with texture, flat areas and 0 / 255 runs (the int16 truncation and clip paths of the filters)"""
    g = rng(seed)
    f = g.integers(0, 256, (h, w), dtype=np.uint8)
    f[h // 3:h // 3 + 20, :] = np.where(g.integers(0, 2, (20, w)) > 0, 255, 0)
    f[:, w // 2:w // 2 + 9] = 128
    return f


def strided(frame, extra_w, extra_h):
    """frame inside a wider and taller allocation whose padding is unlike the edge pixels: 255 - the nearest edge pixel"""
    h, w = frame.shape
    plane = np.empty((h + extra_h, w + extra_w), dtype=np.uint8)
    plane[:h, :w] = frame
    plane[:h, w:] = 255 - frame[:, -1:]
    plane[h:, :] = 255 - plane[h - 1:h, :]
    return plane


# ------------------------------------------------------------------ descriptor lists
def window_x(kind_taps, w, ref_w, where, g):
    """x of a block of width w: 'in' interior, 'edge' on the threshold where the window fits inside ref_w but its
    dword-rounded fetch does not (when the window width is not a multiple of 4), 'out' far outside a border"""
    off = kind_taps // 2 - 1
    ww = w + kind_taps - 1
    if where == "in":
        return int(g.integers(off + 1, ref_w - ww + off - 4))
    if where == "edge":
        return ref_w - ww + off
    return int(g.choice([-w - int(g.integers(10, 60)), ref_w + int(g.integers(10, 60)), -off - 1, ref_w - w + 2]))


def chunk_list(kind, ref_w, ref_h, seed, count=CHUNK_COUNT):
    """sample descriptors for the chunked path: every 64-slot window mixes small and big blocks; every third window holds
    42 big blocks (slots 1, 2, 4, 5, ... up to 62); big blocks alternate shape and interior / clamped windows; the last
    descriptor is big"""
    g = rng(seed)
    luma = kind.startswith("luma")
    taps, nfrac = (8, 4) if luma else (4, 8)
    big, small = (LUMA_BIG, LUMA_SMALL) if luma else (CHROMA_BIG, CHROMA_SMALL)
    out, nb = [], 0
    for i in range(count):
        slot, win = i % 64, i // 64
        is_big = (slot % 3 != 0) if win % 3 == 0 else (slot % 4 == 1)
        if i == count - 1:
            is_big = True
        if is_big:
            w, h = big[nb % len(big)]
            where = ("in", "out", "in", "edge")[nb % 4]
            nb += 1
        else:
            w, h = small[int(g.integers(len(small)))]
            where = ("in", "in", "out", "edge")[int(g.integers(4))]
        x = window_x(taps, w, ref_w, where, g)
        y = window_x(taps, h, ref_h, where if where != "edge" else "in", g)
        out.append((x, y, int(g.integers(nfrac)), int(g.integers(nfrac)), w, h))
    return np.array(out, dtype=np.int32)


def ctu_pus(W, H, seed, ctu=64):
    """the PUs of a random CU quadtree per CTU with random partitions (AMP / SMP included); CUs that cross the bottom or right
    edge of the frame are split"""
    g = rng(seed)
    pus = []

    def cu(x, y, s):
        if x >= W or y >= H:
            return
        if x + s > W or y + s > H or (s > 8 and g.random() < 0.55):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    cu(x + dx, y + dy, s // 2)
            return
        q = s // 4
        parts = [[(0, 0, s, s)], [(0, 0, s, s // 2), (0, s // 2, s, s // 2)], [(0, 0, s // 2, s), (s // 2, 0, s // 2, s)]]
        if s >= 16:
            parts += [[(0, 0, s, q), (0, q, s, s - q)], [(0, 0, s, s - q), (0, s - q, s, q)],
                      [(0, 0, q, s), (q, 0, s - q, s)], [(0, 0, s - q, s), (s - q, 0, q, s)]]
        for (px, py, pw, ph) in parts[int(g.integers(len(parts)))]:
            pus.append((x + px, y + py, pw, ph))
    for cy in range(0, H, ctu):
        for cx in range(0, W, ctu):
            cu(cx, cy, ctu)
    return np.array(pus, dtype=np.int32)


def mc_lists(W, H, seed):
    """one motion-compensation pass: (luma blocks, chroma blocks) of every PU with a random quarter-pel vector, about one
    in eight pointing off the frame"""
    g = rng(seed)
    pus = ctu_pus(W, H, seed)
    luma, chroma = [], []
    for (x, y, w, h) in pus:
        if g.random() < 0.125:
            tx = int(g.integers(-w - 100, W + 100))
            ty = int(g.integers(-h - 100, H + 100))
            mvx, mvy = 4 * (tx - x) + int(g.integers(4)), 4 * (ty - y) + int(g.integers(4))
        else:
            mvx, mvy = int(g.integers(-160, 161)), int(g.integers(-160, 161))
        luma.append((x + (mvx >> 2), y + (mvy >> 2), mvx & 3, mvy & 3, w, h))
        chroma.append((x // 2 + (mvx >> 3), y // 2 + (mvy >> 3), mvx & 7, mvy & 7, w // 2, h // 2))
    return pus, np.array(luma, dtype=np.int32), np.array(chroma, dtype=np.int32)


# ------------------------------------------------------------------ launches
def sample_gpu(env, kind, plane, ref_w, ref_h, blocks, offs, n_elems):
    """kvz_hip_sample_*_batch on `plane` (stride plane.shape[1]) into a CANARY-filled buffer of n_elems; returns it"""
    api, _lib, L = env
    DeviceBuffer = api.DeviceBuffer
    dt = np.int16 if kind.endswith("14") else np.uint8
    init = np.full(n_elems * np.dtype(dt).itemsize, CANARY, np.uint8)
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    r, d, o = DeviceBuffer.from_numpy(plane), DeviceBuffer.from_numpy(blocks), DeviceBuffer.from_numpy(np.asarray(offs, np.uint64))
    dst = DeviceBuffer.from_numpy(init)
    f = L.kvz_hip_sample_luma_batch if kind.startswith("luma") else L.kvz_hip_sample_chroma_batch
    _lib.check(f(r.ptr, plane.shape[1], ref_w, ref_h, d.ptr, o.ptr, blocks.shape[0], int(kind.endswith("14")), dst.ptr, None),
               "sample %s" % kind)
    return dst.to_numpy(dt, (n_elems,))


def sample_oracle(kind, frame, blocks, offs, n_elems):
    """the oracle on the edge-padded frame into the same CANARY-filled layout"""
    dt = np.int16 if kind.endswith("14") else np.uint8
    out = np.full(n_elems * np.dtype(dt).itemsize, CANARY, np.uint8).view(dt)
    return O.sample_many(kind, np.pad(frame, PAD, mode="edge"), PAD, blocks, offs, out)


def packed(blocks):
    sizes = blocks[:, 4].astype(np.int64) * blocks[:, 5]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return offs[:-1].astype(np.uint64), int(offs[-1])


def assert_blocks_equal(got, want, blocks, offs, what):
    if np.array_equal(got, want):
        return
    for i, (b, o) in enumerate(zip(blocks, offs)):
        n = max(0, int(b[4]) * int(b[5]))
        if not np.array_equal(got[int(o):int(o) + n], want[int(o):int(o) + n]):
            raise AssertionError("%s: descriptor %d %s differs first" % (what, i, tuple(int(v) for v in b)))
    bad = np.flatnonzero(got != want)
    raise AssertionError("%s: %d elements outside the blocks changed, first at %d" % (what, bad.size, bad[0]))


_CHUNK_CACHE = {}


def chunk_case(kind):
    """(frame, blocks, offs, n, want) of chunk_list for `kind`, computed once per module"""
    if kind not in _CHUNK_CACHE:
        luma = kind.startswith("luma")
        frame = frame_of(141, 203, 7) if luma else frame_of(71, 101, 8)
        blocks = chunk_list(kind, frame.shape[1], frame.shape[0], 11 + KINDS.index(kind) // 2)
        offs, n = packed(blocks)
        _CHUNK_CACHE[kind] = (frame, blocks, offs, n, sample_oracle(kind, frame, blocks, offs, n))
    return _CHUNK_CACHE[kind]


# ------------------------------------------------------------------ 1. sampling through every branch
@pytest.mark.parametrize("min_wgs", [-1, 0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_sample_chunked_lists(env, knobs, kind, min_wgs):
    """chunk 4 (default knob, 16421 descriptors), 1 (knob 0) and 64 (knob 1); luma also with the 8x8 one-wave path off"""
    frame, blocks, offs, n, want = chunk_case(kind)
    big = (blocks[:, 4] > 16) | (blocks[:, 5] > 16)
    assert big[-1] and big.reshape(-1)[:len(big) // 64 * 64].reshape(-1, 64).sum(1).max() > 32
    knobs(wg_chunk_min_wgs=min_wgs)
    for s8w in ((1, 0) if kind.startswith("luma") else (-1,)):
        knobs(sample8_wave=s8w)
        got = sample_gpu(env, kind, frame, frame.shape[1], frame.shape[0], blocks, offs, n)
        assert_blocks_equal(got, want, blocks, offs, "%s wg_chunk_min_wgs=%d sample8_wave=%d" % (kind, min_wgs, s8w))


# ------------------------------------------------------------------ 2. stride and placement
@pytest.mark.parametrize("min_wgs", [-1, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_sample_stride_placement_and_unsupported(env, knobs, kind, min_wgs):
    """a plane with stride > ref_w and poisoned padding; outputs shuffled against list order, the first at an odd offset,
    gaps of 1..7 canary elements; unsupported descriptors between them write nothing"""
    g = rng(20 + KINDS.index(kind))
    luma = kind.startswith("luma")
    frame = frame_of(93, 117, 21) if luma else frame_of(47, 59, 22)
    plane = strided(frame, 13, 6)
    blocks = chunk_list(kind, frame.shape[1], frame.shape[0], 23 + KINDS.index(kind), count=64 * 5 + 11)
    maxw = 64 if luma else 32
    bad = [(0, 8), (8, 0), (-4, 8), (8, -1), (maxw + 1, 8), (8, maxw + 8), (-1, -1), (maxw + 4, maxw + 4)]
    for j, (w, h) in enumerate(bad):
        blocks[7 + 41 * j] = (5, 5, 1, 1, w, h)
    ok = (blocks[:, 4] >= 1) & (blocks[:, 5] >= 1) & (blocks[:, 4] <= maxw) & (blocks[:, 5] <= maxw)
    # layout: a random order of the descriptors' regions, gaps of 1..7, first region at 3; an unsupported descriptor owns
    # max(w * h, 16) elements that must keep the canary
    region = np.where(ok, blocks[:, 4].astype(np.int64) * blocks[:, 5], np.maximum(blocks[:, 4].astype(np.int64) * blocks[:, 5], 16))
    offs = np.zeros(len(blocks), np.uint64)
    at = 3
    for i in g.permutation(len(blocks)):
        offs[i] = at
        at += int(region[i]) + int(g.integers(1, 8))
    n = at + 5
    want = sample_oracle(kind, frame, blocks[ok], offs[ok], n)
    knobs(wg_chunk_min_wgs=min_wgs)
    got = sample_gpu(env, kind, plane, frame.shape[1], frame.shape[0], blocks, offs, n)
    assert_blocks_equal(got, want, blocks, offs, "%s stride %d > ref_w %d" % (kind, plane.shape[1], frame.shape[1]))
    assert (got.view(np.uint8)[:3 * got.itemsize] == CANARY).all()


# ------------------------------------------------------------------ 3. a motion-compensation pass of a 1080p frame
@pytest.fixture(scope="module")
def mc_frame():
    y = frame_of(1080, 1920, 31)
    c = frame_of(540, 960, 32)
    pus, luma, chroma = mc_lists(1920, 1080, 33)
    return y, c, pus, luma, chroma


@pytest.mark.parametrize("kind", KINDS)
def test_sample_frame_scale_motion_compensation(env, mc_frame, kind):
    api = env[0]
    y, c, pus, luma, chroma = mc_frame
    assert (pus[:, 1] + pus[:, 3]).max() == 1080 and (pus[:, 1] >= 1072).any() and ((pus[:, 2] == 16) & (pus[:, 3] == 4)).any() and ((pus[:, 2] == 12) & (pus[:, 3] == 16)).any()
    frame, blocks = (y, luma) if kind.startswith("luma") else (c, chroma)
    if kind.startswith("chroma"):
        assert {(4, 2), (8, 2), (6, 8)} <= set(map(tuple, blocks[:, 4:6].tolist()))
    offs, n = packed(blocks)
    want = sample_oracle(kind, frame, blocks, offs, n)
    got = np.concatenate([b.ravel() for b in api.sample_batch(kind, frame, blocks, ref_w=frame.shape[1], ref_h=frame.shape[0])])
    assert_blocks_equal(got, want, blocks, offs, "%s 1080p pass of %d PUs" % (kind, len(blocks)))


# ------------------------------------------------------------------ 4. fractional search
def frac_gpu(env, pic, plane, ref_w, ref_h, pairs):
    """kvz_hip_search_frac_batch on `plane` (stride plane.shape[1]) with both outputs filled with FLAG_FILL first"""
    api, _lib, L = env
    DeviceBuffer = api.DeviceBuffer
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[0]
    a, b, d = DeviceBuffer.from_numpy(pic), DeviceBuffer.from_numpy(plane), DeviceBuffer.from_numpy(pairs)
    co = DeviceBuffer.from_numpy(np.full((n, 17), FLAG_FILL, np.uint32))
    be = DeviceBuffer.from_numpy(np.full((n, 2), FLAG_FILL, np.uint32))
    _lib.check(L.kvz_hip_search_frac_batch(a.ptr, pic.shape[1], b.ptr, plane.shape[1], ref_w, ref_h, d.ptr, n, co.ptr, be.ptr, None),
               "search_frac")
    return co.to_numpy(np.uint32, (n, 17)), be.to_numpy(np.int32, (n, 2))


def frac_shape_ok(w, h):
    return 4 <= w <= 64 and 4 <= h <= 64 and not ((w | h) & 3) and not ((w & 4) and (h & 4))


def frac_list(ref_w, ref_h, seed, count):
    """frac search pairs: every 64-slot window mixes the small, medium and big kernels' shapes (every third window 42 big
    ones, slots above 32 included), big ones alternate shape and interior / clamped windows, malformed ones at slots 5, 37
    and 50 of every other window, the last descriptor big"""
    g = rng(seed)
    out, nb, nm = [], 0, 0
    for i in range(count):
        slot, win = i % 64, i // 64
        if win % 2 == 0 and slot in (5, 37, 50):
            w, h = FRAC_MALFORMED[nm % len(FRAC_MALFORMED)]
            nm += 1
            out.append((8, 8, 8, 8, w, h))
            continue
        is_big = (slot % 3 != 0) if win % 3 == 0 else (slot % 4 == 1)
        if is_big or i == count - 1:
            w, h = FRAC_BIG[nb % len(FRAC_BIG)]
            where = ("in", "out")[nb % 2]
            nb += 1
        else:
            w, h = (FRAC_SMALL + FRAC_MEDIUM)[int(g.integers(len(FRAC_SMALL) + len(FRAC_MEDIUM)))]
            where = ("in", "out", "in", "edge")[int(g.integers(4))]
        x1, y1 = int(g.integers(0, ref_w - w + 1)), int(g.integers(0, ref_h - h + 1))
        if where == "in":            # the whole 8-pixel margin inside: the dword fetch
            x2, y2 = int(g.integers(4, ref_w - w - 3)), int(g.integers(4, ref_h - h - 3))
        elif where == "edge":        # on a border: the margin just leaves the plane
            x2, y2 = int(g.choice([3, ref_w - w - 3, 0, ref_w - w])), int(g.integers(4, ref_h - h - 3))
        else:                        # far outside a border or corner
            x2 = int(g.choice([-w - int(g.integers(5, 80)), ref_w + int(g.integers(5, 80)), int(g.integers(4, ref_w - w - 3))]))
            y2 = int(g.choice([-h - int(g.integers(5, 80)), ref_h + int(g.integers(5, 80))]))
        out.append((x1, y1, x2, y2, w, h))
    return np.array(out, dtype=np.int32)


def frac_expected(pic, frame, pairs):
    ok = np.array([frac_shape_ok(int(w), int(h)) for w, h in pairs[:, 4:6]])
    costs = np.full((len(pairs), 17), 0xFFFFFFFF, np.uint32)
    best = np.full((len(pairs), 2), -1, np.int32)
    costs[ok], best[ok] = O.search_frac_many(pic, frame, pairs[ok])
    return costs, best


def assert_frac_equal(got, want, pairs, what):
    for a, b, name in ((got[0], want[0], "costs"), (got[1], want[1], "best")):
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, "%s: %s of %d descriptors differ, first %d %s: %s != %s" % (
            what, name, bad.size, bad[0], tuple(pairs[bad[0]]), a[bad[0]].tolist(), b[bad[0]].tolist())


@pytest.fixture(scope="module")
def frac_chunk_case():
    frame = frame_of(150, 211, 41)
    pic = ((frame.astype(np.int32) + np.roll(frame, (1, 3), axis=(0, 1))) // 2).astype(np.uint8)
    pairs = frac_list(frame.shape[1], frame.shape[0], 42, CHUNK_COUNT)
    return frame, pic, strided(frame, 9, 5), pairs, frac_expected(pic, frame, pairs)


@pytest.mark.parametrize("min_wgs", [-1, 0, 1])
def test_search_frac_chunked_lists_and_flags(env, knobs, frac_chunk_case, min_wgs):
    """all three kernels over 16421 descriptors with malformed ones in the chunks, on a plane with stride > ref_w"""
    frame, pic, plane, pairs, want = frac_chunk_case
    wh = pairs[:, 4:6]
    assert set(FRAC_MALFORMED) <= set(map(tuple, wh.tolist()))
    assert ((wh > 32).any(1)).reshape(-1)[:len(wh) // 64 * 64].reshape(-1, 64).sum(1).max() > 32 and (wh[-1] > 32).any()
    knobs(wg_chunk_min_wgs=min_wgs)
    got = frac_gpu(env, pic, plane, frame.shape[1], frame.shape[0], pairs)
    assert_frac_equal(got, want, pairs, "wg_chunk_min_wgs=%d" % min_wgs)


def test_search_frac_every_shape_at_borders(env):
    """each legal shape of the three kernels at every border and corner of the picture, with vectors on the borders and far
    off the plane, on a plane with stride > ref_w, and each malformed shape beside them"""
    frame = frame_of(137, 173, 51)
    pic = frame_of(137, 173, 52)
    W, H = frame.shape[1], frame.shape[0]
    pairs = []
    for (w, h) in FRAC_SMALL + FRAC_MEDIUM + FRAC_BIG:
        for (x, y) in ((0, 0), (W - w, 0), (0, H - h), (W - w, H - h), (W // 3, H // 2)):
            for (x2, y2) in ((x, y), (x - 1, y + 2), (-w - 70, y), (W + 50, H + 60), (4, 4), (W - w - 4, H - h - 4), (W - w - 3, 3)):
                pairs.append((x, y, x2, y2, w, h))
        pairs.append((9, 9, 9, 9) + FRAC_MALFORMED[len(pairs) % len(FRAC_MALFORMED)])
    pairs = np.array(pairs, dtype=np.int32)
    got = frac_gpu(env, pic, strided(frame, 11, 7), W, H, pairs)
    assert_frac_equal(got, frac_expected(pic, frame, pairs), pairs, "border shapes")


def test_search_frac_frame_scale(env, mc_frame):
    """every PU of the 1080p quadtree with an integer vector, default knobs, through api.search_frac_batch"""
    api = env[0]
    y, _, pus, _, _ = mc_frame
    g = rng(61)
    pic = np.roll(y, (2, -3), axis=(0, 1))
    keep = np.array([frac_shape_ok(int(w), int(h)) for w, h in pus[:, 2:4]])
    p = pus[keep]
    mv = g.integers(-24, 25, (len(p), 2))
    far = g.random(len(p)) < 0.05
    mv[far] = g.integers(-300, 301, (int(far.sum()), 2))
    pairs = np.stack([p[:, 0], p[:, 1], p[:, 0] + mv[:, 0], p[:, 1] + mv[:, 1], p[:, 2], p[:, 3]], axis=1).astype(np.int32)
    got = api.search_frac_batch(pic, y, pairs, ref_w=1920, ref_h=1080)
    assert_frac_equal(got, O.search_frac_many(pic, y, pairs), pairs, "1080p pass of %d PUs" % len(pairs))


# ------------------------------------------------------------------ 5. intra_rough_waves
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("log2_width", [2, 3, 4, 5])
def test_intra_rough_waves(env, knobs, log2_width, waves):
    """both workgroup sizes at every PU size, with and without SAD; counts leave the last workgroup ragged"""
    api = env[0]
    per_wg = {2: 64, 3: 64, 4: 16, 5: 4}[log2_width]
    count = 3 * per_wg + per_wg // 2 + 1
    refs = intra_ref_cases(log2_width, count, 700 + log2_width)
    g = rng(710 + log2_width)
    n = 1 << log2_width
    base = O.intra_predict_batch(refs, log2_width, [int(g.integers(0, 35))])[:, 0, :].astype(np.int32)
    orig = np.clip(base + g.integers(-12, 13, (count, n * n)), 0, 255).astype(np.uint8)
    orig[::5] = g.integers(0, 256, (len(orig[::5]), n * n), dtype=np.uint8)
    knobs(intra_rough_waves=waves)
    for fb in (1, 0):
        want_satd, want_sad = O.intra_rough_costs_batch(refs, log2_width, orig, fb)
        satd, sad = api.intra_rough_batch(refs, log2_width, orig, 1 | (fb << 1), with_sad=True)
        np.testing.assert_array_equal(satd, want_satd, err_msg="satd waves=%d fb=%d" % (waves, fb))
        np.testing.assert_array_equal(sad, want_sad, err_msg="sad waves=%d fb=%d" % (waves, fb))
        np.testing.assert_array_equal(api.intra_rough_batch(refs, log2_width, orig, 1 | (fb << 1)), want_satd)

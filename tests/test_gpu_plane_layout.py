"""GPU: every entry of the C ABI that takes planes as (pointer, stride, size), on planes that are rectangles inside larger buffers.

The expected value is always the oracle (tests/oracle_lib.py) on the COMPACT planes; the GPU gets the same planes embedded in
poisoned buffers (patterns.embed_plane) on three layouts (patterns.plane_layout):
  A (padded): base 16-byte aligned, stride = width + 4k, not a multiple of 16 more than the width;
  B (offset): plane 4 bytes into the rows and one row down, stride a multiple of 4 but not of 16;
  C (odd):    plane 1 byte into the rows, odd stride.
In every call the planes have different strides (pic < ref < ref1, rec < new_rec, stride_c != stride_y / 2), and every buffer
is long enough for the LARGEST stride of its call, so a kernel that clamps against the stride instead of the width, swaps two
strides or assumes an aligned base gets a wrong number from the poison, never an address outside an allocation.  All results
are integers and compared exactly.  kvz_hip_deblock_frame documents 4-byte alignment: layout C checks its refusal instead.
kvz_hip_intra_build_reference_batch is not here: test_gpu_parity.py::test_intra_build_reference already reads a plane whose
stride exceeds the picture width by 24 random bytes."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from patterns import (ME_RESULT, PLANE_LAYOUTS, REG_SAD_DIMS, deblock_case, deblock_params, embed_plane, me_cabac_states, me_frames,
                      me_params, me_pus_in_tile, me_random_pus, plane_layout, rng, sao_records)

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("layout", PLANE_LAYOUTS)
KVZ_HIP_ERR_INVALID = -2
ME_FIELDS = ("mv", "cost", "bitcost", "merged", "merge_idx", "mv_cand", "reserved")


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


def _lib0():
    from kvazaar_amd import _lib
    return _lib.init(0)


def embed_call(layout, planes, seed, offsets=None):
    """The compact `planes` of ONE call on `layout`: plane k gets the k-th stride of the layout (so they all differ and grow with
    k) and a buffer long enough for the largest of them.  offsets: per plane, rows added to the layout's `top`.
    -> list of patterns.EmbeddedPlane"""
    geo = [plane_layout(layout, p.shape[1], k) for k, p in enumerate(planes)]
    span = max(s for s, _, _ in geo)
    out = [embed_plane(p, s, left, top + (offsets[k] if offsets else 0), seed + 17 * k, span=span) for k, (p, (s, left, top)) in enumerate(zip(planes, geo))]
    strides = [e.stride for e in out]
    assert len(set(strides)) == len(strides) and strides == sorted(strides)
    for e in out:
        assert e.offset % 16 == 0 if layout == "A" else (e.offset % 4 == 0 and e.offset % 16 != 0 and e.stride % 16 != 0) if layout == "B" else \
            (e.offset % 2 == 1 and e.stride % 2 == 1)
    return out


def view(api, e):
    return api.PlaneView(e.buf, e.width, e.height, e.left, e.top)


# ------------------------------------------------------------------ pair entries
PW, PH = 96, 72                                              # the planes of the pair entries
MOVES = ((0, 0), (3, -2), (-5, 4), (-100, 1), (100, -1), (2, -80), (-2, 80), (-100, -80), (100, 80), (-7, -7), (9, 6))   # inside; beyond each edge; corners


@functools.lru_cache(maxsize=None)
def pair_case():
    """-> planes, per entry (pairs, expected), and the 4097 8x8 pairs with their expected values"""
    g = rng(4100)
    pic = g.integers(0, 256, (PH, PW), dtype=np.uint8)
    ref = np.clip(np.roll(pic, (1, -2), (0, 1)).astype(np.int32) + g.integers(-20, 21, (PH, PW)), 0, 255).astype(np.uint8)

    def inside(w, h):
        return int(g.integers(0, PW - w + 1)), int(g.integers(0, PH - h + 1))

    def moved(dims, n):
        out = []
        for i in range(n):
            w, h = dims[i % len(dims)]
            x1, y1 = inside(w, h)
            dx, dy = MOVES[(i // len(dims) + i) % len(MOVES)]
            out.append((x1, y1, x1 + dx, y1 + dy, w, h))
        return out

    sad_dims = REG_SAD_DIMS + [(64, 63), (1, 1), (7, 3), (13, 5)]
    satd_dims = [(8, 8), (16, 16), (64, 64), (4, 4), (16, 8), (32, 32), (12, 16), (8, 4)]
    reg = [inside(w, h) + inside(w, h) + (w, h) for i in range(198) for (w, h) in (sad_dims[i % len(sad_dims)],)]
    ssd = [inside(w, w) + inside(w, w) + (w, w) for i in range(200) for w in ((8, 16, 64, 4, 32)[i % 5],)]
    sad, satd = moved(sad_dims, 198), moved(satd_dims, 200)
    small = moved([(8, 8)], 4097)                             # the grid-stride chunk kernels take batches above 4096
    small_in = [inside(8, 8) + inside(8, 8) + (8, 8) for _ in range(4097)]

    def want(kind, pairs):
        if kind == "reg_sad":
            return [O.reg_sad(pic, ref, p[1] * PW + p[0], p[3] * PW + p[2], p[4], p[5], PW, PW) for p in pairs]
        if kind == "ssd":
            return [O.pixels_calc_ssd(pic, p[1] * PW + p[0], ref, p[3] * PW + p[2], PW, PW, p[4]) for p in pairs]
        return [O.image_calc(kind, pic, ref, *p) for p in pairs]

    cases = {"reg_sad": (reg, small_in), "image_calc_sad": (sad, small), "image_calc_satd": (satd, small), "pixels_calc_ssd": (ssd, small_in)}
    kinds = {"reg_sad": "reg_sad", "image_calc_sad": "sad", "image_calc_satd": "satd", "pixels_calc_ssd": "ssd"}
    return pic, ref, {e: (a, want(kinds[e], a), b, want(kinds[e], b)) for e, (a, b) in cases.items()}


@LAYOUTS
@pytest.mark.parametrize("entry", ["reg_sad", "image_calc_sad", "image_calc_satd", "pixels_calc_ssd"])
def test_pair_entry(api, entry, layout):
    """about 200 pairs through the wave-per-descriptor kernel and, with the knob, through the grid-stride one; then 4097 8x8 pairs,
    which always take the grid-stride chunk kernel"""
    pic, ref, cases = pair_case()
    pairs, want, small, want_small = cases[entry]
    p, r = (view(api, e) for e in embed_call(layout, [pic, ref], 10))
    f = getattr(api, entry + "_batch")
    for knob in (1, 0):
        with api.tuned(pair_wave_kernel=knob):
            np.testing.assert_array_equal(f(p, r, pairs), want, err_msg="%s layout %s pair_wave_kernel %d" % (entry, layout, knob))
    np.testing.assert_array_equal(f(p, r, small), want_small, err_msg="%s layout %s, 4097 8x8 pairs" % (entry, layout))


# ------------------------------------------------------------------ satd_any_size_quad
QUAD_PRED_STRIDE, QUAD_ITEM_STRIDE = 80, 80 * 64 + 48


@functools.lru_cache(maxsize=None)
def quad_case():
    g = rng(4200)
    orig = g.integers(0, 256, (PH, PW), dtype=np.uint8)
    dims = [(w, h) for w in (4, 8, 12, 16, 24, 32, 64) for h in (4, 8, 12, 16, 24, 32, 64)]     # incl. the widths of the reference's quirk
    preds = g.integers(0, 256, (len(dims) * 4, 64, 64), dtype=np.uint8)
    pairs = [(11 + 4 * (i % 3), 3 + (i % 5), 0, 0, w, h) for i, (w, h) in enumerate(dims)]
    want = np.array([O.satd_any_size_quad(w, h, [preds[4 * i + k] for k in range(4)], 64, orig, y * PW + x, PW)
                     for i, (x, y, _, _, w, h) in enumerate(pairs)])
    # the predictions again with rows 80 bytes apart and items 80 * 64 + 48 bytes apart, poison in every gap
    wide = rng(4201).integers(0, 256, (len(preds), QUAD_ITEM_STRIDE), dtype=np.uint8)
    for i in range(len(preds)):
        rows = wide[i, :QUAD_PRED_STRIDE * 64].reshape(64, QUAD_PRED_STRIDE)      # a view of the item
        rows[:, :64] = preds[i]
        rows[:, 64] = preds[i][:, 63] ^ 0x80
    return orig, preds, wide, pairs, want


@LAYOUTS
def test_satd_any_size_quad(api, layout):
    orig, preds, wide, pairs, want = quad_case()
    o = view(api, embed_call(layout, [orig], 20)[0])
    np.testing.assert_array_equal(api.satd_any_size_quad_batch(preds.reshape(len(preds), -1), o, pairs), want, err_msg="layout %s" % layout)
    np.testing.assert_array_equal(api.satd_any_size_quad_batch(wide, o, pairs, pred_stride=QUAD_PRED_STRIDE, pred_item_stride=QUAD_ITEM_STRIDE),
                                  want, err_msg="layout %s, pred_stride 80" % layout)


# ------------------------------------------------------------------ ctu_sad_grid
@functools.lru_cache(maxsize=None)
def ctu_case():
    g = rng(4300)
    H, W = 72, 136                                            # full CTU columns, a ragged column (8 px), a ragged row (8 px)
    ref = g.integers(0, 256, (H, W), dtype=np.uint8)
    pic = np.clip(np.roll(ref, (2, -3), axis=(0, 1)).astype(np.int32) + g.integers(-5, 6, (H, W)), 0, 255).astype(np.uint8)
    # search centres that push the window across the left, right, top and bottom edge, and two corners
    ctus = [(x, y, mvx, mvy) for y in range(0, H, 64) for x in range(0, W, 64)
            for (mvx, mvy) in ((0, 0), (3, -2), (-70, 5), (80, -3), (4, -75), (-6, 75), (-140, -80), (150, 90))]
    grid = [(dx, dy) for dy in (-6, -3, 0, 3, 6) for dx in (-6, -3, 0, 3, 6)]
    hexbs = [(0, 0), (-2, 0), (-1, -2), (1, -2), (2, 0), (1, 2), (-1, 2), (1, 0), (0, 1), (-1, 0), (0, -1)]
    wide = [(-64, -64), (64, 64), (17, -33), (-1, 1), (65, 0), (0, -100)]
    offs = (grid, hexbs, wide)
    return pic, ref, ctus, offs, [O.ctu_sad_grid(pic, ref, ctus, o) for o in offs]


@LAYOUTS
def test_ctu_sad_grid(api, layout):
    pic, ref, ctus, offs, want = ctu_case()
    p, r = (view(api, e) for e in embed_call(layout, [pic, ref], 30))
    for k, o in enumerate(offs):
        np.testing.assert_array_equal(api.ctu_sad_grid_batch(p, r, ctus, o), want[k], err_msg="layout %s offsets %d" % (layout, k))


# ------------------------------------------------------------------ search_pu
ME_SIZES = ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (64, 32), (24, 32), (32, 8),     # 2Nx2N, SMP
            (8, 4), (4, 8), (16, 4), (4, 16), (16, 12), (12, 16), (32, 24), (64, 16))                           # AMP
# one run per kernel family: (name, me_params arguments, tuning knobs or None)
ME_RUNS = (("hexbs", dict(fme_level=4), None), ("dia", dict(algorithm=1), None), ("tz", dict(algorithm=2), None),
           ("full, full_qsad 0", dict(algorithm=3, search_range=8), dict(full_qsad=0)),
           ("full, full_qsad 1", dict(algorithm=3, search_range=8), dict(full_qsad=1)),
           ("mv_rdo", dict(mv_rdo=1, refs_before=3, ref_idx=2, lambda_cost=11), None),
           ("tile", dict(mv_constraint=4, tile=(0, 64, 192, 64), lambda_cost=11), None))


def me_pus(seed, prm, motion):
    pus = me_random_pus(192, 128, 40, seed, hint=(-4 * motion[0] + 2, -4 * motion[1]), sizes=ME_SIZES)
    pus["x"] = np.minimum((pus["x"] // 4) * 4 + 4 * (np.arange(len(pus)) % 2), 192 - pus["width"])      # also off the 8-pixel grid
    return me_pus_in_tile(pus, prm)


@functools.lru_cache(maxsize=None)
def me_case():
    motion = (3, -2)
    pic, ref = me_frames(192, 128, 4400, motion)
    cab = me_cabac_states(9, 44)
    runs = []
    for k, (name, cfg, knob) in enumerate(ME_RUNS):
        prm = me_params(**cfg)
        pus = me_pus(4410 + (3 if "full" in name else k), prm, motion)
        cabac = None
        if cfg.get("mv_rdo"):
            pus["reserved"] = np.arange(len(pus)) % len(cab)
            cabac = cab
        runs.append((name, prm, knob, pus, cabac, O.search_pu_batch(pic, ref, pus, prm, cabac=cabac)))
    return pic, ref, runs


def assert_me_equal(got, want, msg):
    got = got.view(ME_RESULT).reshape(-1)
    for f in ME_FIELDS:
        np.testing.assert_array_equal(got[f], want[f] if f != "reserved" else np.zeros(len(got), np.int32), err_msg="%s: %s" % (msg, f))


@LAYOUTS
def test_search_pu(api, layout):
    """hexbs, dia, tz, the exhaustive search, --mv-rdo and a constrained tile.  No layout is refused: the kernels of this entry read the
    current block and the reference with byte-addressed vector loads (only the search service, which owns its planes, reads the
    block with scalar dword loads)"""
    pic, ref, runs = me_case()
    p, r = (view(api, e) for e in embed_call(layout, [pic, ref], 40))
    for name, prm, knob, pus, cabac, want in runs:
        with api.tuned(**(knob or {})):
            got = api.search_pu_batch(p, r, pus, prm, cabac=cabac)
        assert_me_equal(got, want, "layout %s, %s" % (layout, name))


@functools.lru_cache(maxsize=None)
def me_multi_case():
    pairs = [me_frames(192, 128, 4500 + k, motion) for k, motion in enumerate(((3, -2), (-7, 5)))]
    runs = []
    for name, cfg in (("hexbs", dict()), ("full", dict(algorithm=3, search_range=8))):
        prm = me_params(**cfg)
        pus = me_pus(4510, prm, (3, -2))
        owner = (np.arange(len(pus)) // 3) % 2
        pus["pad"] = (owner << 2) | (np.arange(len(pus)) % 4)
        want = np.zeros(len(pus), ME_RESULT)
        for k, (pic, ref) in enumerate(pairs):
            sel = np.where(owner == k)[0]
            want[sel] = O.search_pu_batch(pic, ref, pus[sel], prm)
        runs.append((name, prm, pus, want))
    return pairs, runs


@LAYOUTS
def test_search_pu_multi(api, layout):
    """two picture pairs that share the strides; every plane starts at another offset into its buffer"""
    pairs, runs = me_multi_case()
    (sp, _, _), (sr, _, _) = plane_layout(layout, 192, 0), plane_layout(layout, 192, 1)
    pics, refs = [], []
    for k, (pic, ref) in enumerate(pairs):
        _, left, top = plane_layout(layout, 192)
        pics.append(embed_plane(pic, sp, left, top + 4 * k, 50 + k, span=sr))
        refs.append(embed_plane(ref, sr, left, top + 4 * (1 - k), 60 + k, span=sr))
    assert len({e.offset for e in pics + refs}) == 4 and sp < sr
    pv, rv = [view(api, e) for e in pics], [view(api, e) for e in refs]
    for name, prm, pus, want in runs:
        assert_me_equal(api.search_pu_multi_batch(pv, rv, pus, prm), want, "layout %s, %s" % (layout, name))


# ------------------------------------------------------------------ bipred_cost
@functools.lru_cache(maxsize=None)
def bipred_case():
    g = rng(4600)
    pic, ref0 = me_frames(192, 128, 12, (2, -1))
    _, ref1 = me_frames(192, 128, 13, (-3, 2))
    ref1 = np.where(g.integers(0, 40, ref1.shape) == 0, 255, ref1).astype(np.uint8)
    cands, k = [], 0
    for (w, h) in ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (32, 64), (24, 8), (8, 4), (4, 8), (16, 4), (4, 16), (16, 12), (12, 16)):
        for _ in range(3):
            x = int(g.integers(0, 3)) * 64 + int(g.integers(0, (64 - w) // 4 + 1)) * 4
            y = int(g.integers(0, 2)) * 64 + int(g.integers(0, (64 - h) // 4 + 1)) * 4
            big = 400 if k % 5 == 4 else 24                          # every fifth pair leaves the frame
            mv0, mv1 = g.integers(-big, big + 1, 2), g.integers(-big, big + 1, 2)
            if k % 3 == 0:
                mv0 = (mv0 // 4) * 4                                 # integer vectors: the edge-clamped pixels << 6
            if k % 4 == 1:
                mv1 = (mv1 // 4) * 4
            cands.append((x, y, w, h, int(mv0[0]), int(mv0[1]), int(mv1[0]), int(mv1[1])))
            k += 1
    want = [O.bipred_luma_satd(pic, ref0, ref1, c[0], c[1], c[2], c[3], c[4:6], c[6:8])[0] for c in cands]
    return pic, ref0, ref1, cands, want


@LAYOUTS
def test_bipred_cost(api, layout):
    pic, ref0, ref1, cands, want = bipred_case()
    p, r0, r1 = (view(api, e) for e in embed_call(layout, [pic, ref0, ref1], 70))
    np.testing.assert_array_equal(api.bipred_cost_batch(p, r0, r1, cands), want, err_msg="layout %s" % layout)


# ------------------------------------------------------------------ deblock_frame
DEBLOCK_RUNS = (("P slice", dict(qp=34)), ("B slice, per_cu_qp", dict(qp=36, slice_is_b=1, per_cu_qp=1)), ("chroma 0", dict(qp=40, chroma=0)))


@functools.lru_cache(maxsize=None)
def deblock_cases():
    out = []
    for k, (name, cfg) in enumerate(DEBLOCK_RUNS):
        prm = deblock_params(**cfg)
        chroma = bool(prm["chroma"][0])
        y, u, v, cus = deblock_case(72, 72, 4700 + k, slice_is_b=int(prm["slice_is_b"][0]), qp=int(prm["qp"][0]), intra_share=0.35)
        if not chroma:
            u = v = None
        want = O.deblock_frame(y, u, v, cus, prm)
        assert (want[0] != y).any()
        out.append((name, prm, (y, u, v), cus, want))
    return out


def deblock_planes(layout, planes, seed):
    """Y with the layout's first stride; U and V share its second one for their width (never stride_y / 2)"""
    y, u, v = planes
    sy, left, top = plane_layout(layout, 72, 0)
    sc, _, _ = plane_layout(layout, 36, 1)
    assert 2 * sc > sy and 2 * sc != sy
    return [embed_plane(p, s, left, top, seed + k, span=sy) if p is not None else None for k, (p, s) in enumerate(((y, sy), (u, sc), (v, sc)))]


@pytest.mark.parametrize("layout", ["A", "B"])
def test_deblock_frame(api, layout):
    """a CTU plus a ragged row and column, filtered in place: the planes equal the oracle's, the bytes around them are untouched"""
    for k, (name, prm, planes, cus, want) in enumerate(deblock_cases()):
        emb = deblock_planes(layout, planes, 80 + 10 * k)
        got = api.deblock_frame(*[view(api, e) if e is not None else None for e in emb], cus, prm)
        for c, e in enumerate(emb):
            if e is None:
                assert got[c] is None
                continue
            np.testing.assert_array_equal(e.crop(got[c]), want[c], err_msg="layout %s, %s, plane %d" % (layout, name, c))
            assert e.poison_intact(got[c]), "layout %s, %s: bytes around plane %d were written" % (layout, name, c)


def test_deblock_frame_refuses_layout_C(api):
    """planes and strides must be 4-byte aligned (include/kvz_hip.h): KVZ_HIP_ERR_INVALID with the entry's name, nothing written --
    for all planes on layout C, and for an aligned luma plane with chroma on layout C"""
    L = _lib0()
    for name, prm, planes, cus, _ in deblock_cases():
        chroma = bool(prm["chroma"][0])
        for luma_layout in ("C", "A") if chroma else ("C",):
            emb = deblock_planes("C", planes, 90)
            emb[0] = deblock_planes(luma_layout, planes, 90)[0]
            dev = [api.DeviceBuffer.from_numpy(e.buf) if e is not None else None for e in emb]
            dc = api.DeviceBuffer.from_numpy(np.ascontiguousarray(cus).view(np.uint8))
            rc = L.kvz_hip_deblock_frame(dev[0].ptr + emb[0].offset, emb[0].stride, dev[1].ptr + emb[1].offset if chroma else None,
                                         dev[2].ptr + emb[2].offset if chroma else None, emb[1].stride if chroma else 0, 72, 72, dc.ptr,
                                         prm.ctypes.data, None)
            assert rc == KVZ_HIP_ERR_INVALID, "%s, luma on layout %s" % (name, luma_layout)
            assert b"kvz_hip_deblock_frame" in L.kvz_hip_last_error()
            assert L.kvz_hip_stream_sync(None) == 0
            for e, d in zip(emb, dev):
                if e is not None:
                    np.testing.assert_array_equal(d.to_numpy(np.uint8, e.buf.shape), e.buf, err_msg="%s: a refused call wrote" % name)


# ------------------------------------------------------------------ sao_reconstruct_color
@functools.lru_cache(maxsize=None)
def sao_case(color):
    g = rng(4800 + color)
    H, W, n = 40, 72, 64
    plane = g.integers(0, 256, (H, W), dtype=np.uint8)
    plane[8:30, 10:60] = np.where(g.integers(0, 2, (22, 50)) > 0, 252, 2)
    canary = rng(4810 + color).integers(0, 256, (H, W), dtype=np.uint8)
    grid = []
    for y in range(0, H, n):
        for x in range(0, W, n):
            x0, y0, x1, y1 = max(x, 1), max(y, 1), min(x + n, W - 1), min(y + n, H - 1)
            grid.append((x0, y0, x1 - x0, y1 - y0))
    infos = sao_records(4, 9 + color)                         # 0: band, 1: edge, 2: none, 3: edge, horizontal (the skipped descriptor's)
    infos[2, 0] = 0
    infos[3, 1] = 0
    # the grid has two blocks: two calls give each of band, edge and none a block.  One more descriptor must be skipped: its class
    # reads the column at x = W, inside the stride but outside the plane
    skipped = (W - 8, 4, 8, 8, 3)
    calls = []
    for rot in (0, 1):
        blocks = [b + ((i + rot) % 3,) for i, b in enumerate(grid)]
        want = canary.copy()
        for (x, y, w, h, idx) in blocks:
            want[y:y + h, x:x + w] = O.sao_reconstruct_color(plane, x, y, w, h, infos[idx], color) if infos[idx, 0] != 0 else plane[y:y + h, x:x + w]
        calls.append((blocks + [skipped], want))
    return plane, canary, infos, calls


@LAYOUTS
@pytest.mark.parametrize("color", [0, 1, 2])
def test_sao_reconstruct_color(api, color, layout):
    plane, canary, infos, calls = sao_case(color)
    rec, new = embed_call(layout, [plane, canary], 100 + color)
    for k, (blocks, want) in enumerate(calls):
        got = api.sao_reconstruct_color_batch(view(api, rec), blocks, infos, color, new_rec=view(api, new))
        np.testing.assert_array_equal(new.crop(got), want, err_msg="layout %s colour %d call %d" % (layout, color, k))
        assert new.poison_intact(got), "layout %s colour %d call %d: the padding of new_rec was written" % (layout, color, k)

"""The TUs of tests/golden/rdoq.npz: seeded and directed coefficient blocks for kvz_hip_rdoq_batch over all widths, both types, the allowed
scans, intra and inter, tr_depth 0..3, QP 4..51, sign hiding on and off and flat and default scaling lists.  cases() builds them; the
results come from the compiled reference (tests/gen_rdoq_golden.py).  TEST INFRASTRUCTURE.

A context set is (184 context bytes, qp, lambda): what one kvz_hip_coeff_ctx / kvz_hip_rdoq_state pair carries.  The bytes are
kvz_init_contexts of the set's QP for a P or an I slice (base_contexts(), stored in the fixture because only the reference produces
them) with a quarter of them replaced by values in 0..125; lambda = 0.57 * 2 ** ((qp - 12) / 3).

A case is (coef int16 [width * width], width, type, scan_mode, block_type, tr_depth, set index, configuration index); CONFIGS lists the
(signhide, default_lists) pairs: a call of the batch entry has one signhide and one pair of tables.

Seeded coefficients have an amplitude of about 3 quantiser steps at DC that decays along x + y, with occasional 2.5-fold outliers: levels
of 0..3 nearly everywhere, where RDOQ decides differently from rounding."""
import numpy as np

CONFIGS = ((1, 0), (0, 0), (1, 1), (0, 1))
QPS = tuple(range(4, 52))
N_SETS = len(QPS)
SEED = 20241107
SEEDED = ((4, 400), (8, 300), (16, 100), (32, 40))
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)      # scalinglist.c:66: a flat list's factor per qp % 6
CHROMA_SCALE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32,
                33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51)


def base_contexts(init_contexts):
    """uint8 [N_SETS, 184]: init_contexts(qp, slice type) -- tests/ref_rdoq.py -- of every set's QP, P and I slices alternating"""
    return np.stack([np.asarray(init_contexts(qp, (1, 2)[k % 2]), dtype=np.uint8) for k, qp in enumerate(QPS)])


def lambda_of(qp):
    return 0.57 * 2.0 ** ((qp - 12) / 3.0)


def context_sets(base, seed=SEED):
    """(dumps uint8 [N_SETS, 184], qps int8 [N_SETS], lambdas float64 [N_SETS])"""
    g = np.random.default_rng(seed)
    dumps = np.array(base, dtype=np.uint8)
    assert dumps.shape == (N_SETS, 184)
    swap = g.random(dumps.shape) < 0.25
    dumps[swap] = g.integers(0, 126, int(swap.sum()))
    return dumps, np.array(QPS, dtype=np.int8), np.array([lambda_of(q) for q in QPS], dtype=np.float64)


def _scans(width):
    return (0, 1, 2) if width <= 8 else (0,)


def step_of(width, type_, qp):
    """the quantiser step of a flat list in coefficient units: 2 ** q_bits / factor"""
    qps = qp if type_ == 0 else CHROMA_SCALE[qp]
    q_bits = 14 + qps // 6 + (15 - 8 - (width.bit_length() - 1))
    return float(1 << q_bits) / QUANT_SCALES[qps % 6]


def seeded_tu(g, width, type_, qp, steps=3.0):
    yy, xx = np.divmod(np.arange(width * width), width)
    amp = steps * step_of(width, type_, qp) * np.exp(-(xx + yy) / (width / 2.0))
    c = g.normal(0.0, 1.0, width * width) * amp * np.where(g.random(width * width) < 0.04, 2.5, 1.0)
    return np.clip(np.rint(c), -32768, 32767).astype(np.int16)


def seeded(g, widths, per_width):
    """seeded cases: every combination of type, scan, block type and depth comes round; 32x32 is luma only"""
    out = []
    for width, count in zip(widths, per_width):
        for k in range(count):
            type_ = 0 if width == 32 else (0, 2)[k % 2]
            scan = _scans(width)[(k // 2) % len(_scans(width))]
            block_type = (1, 2)[(k // 6) % 2]
            tr_depth = (k // 12) % 4
            set_ = int(g.integers(0, N_SETS))
            cfg = (0, 0, 0, 1, 2, 3)[k % 6] if k % 5 else (k // 5) % 4
            out.append((seeded_tu(g, width, type_, QPS[set_], steps=(3.0, 3.0, 1.2, 6.0)[(k // 3) % 4]),
                        width, type_, scan, block_type, tr_depth, set_, cfg))
    return out


def cases(seed=SEED):
    g = np.random.default_rng(seed + 1)
    out = seeded(g, [w for w, _ in SEEDED], [c for _, c in SEEDED])

    def add(c, width, type_, scan, block_type=1, tr_depth=0, set_=None, cfg=0):
        c = np.clip(np.rint(np.asarray(c, dtype=np.float64)), -32768, 32767).astype(np.int16).reshape(width * width)
        out.append((c, width, type_, scan, block_type, tr_depth, int(g.integers(0, N_SETS)) if set_ is None else set_, cfg))

    # ---- directed
    for width in (4, 8, 16, 32):
        n = width * width
        for type_ in ((0,) if width == 32 else (0, 2)):
            for scan in _scans(width):
                for cfg in range(len(CONFIGS)):
                    add(np.zeros(n), width, type_, scan, cfg=cfg)                             # nothing to code: all zero comes out
                for set_ in (3, 20, 40):
                    step = step_of(width, type_, QPS[set_])
                    for pos in (0, n - 1, width - 1, n - width):                             # one coefficient: DC and the corners
                        for v in (0.6, 1.4, -2.6, 9.0):
                            c = np.zeros(n)
                            c[pos] = v * step
                            add(c, width, type_, scan, block_type=1 + (pos & 1), tr_depth=(pos + set_) % 4, set_=set_, cfg=(pos + set_) % 4)
                    # levels far above 48: the Rice parameter climbs to its cap inside one group, the escape code takes its loop
                    c = np.zeros(n)
                    for k, v in enumerate((4, 7, 13, 25, 49, 97, 60, 55, 52, 70, 3, 2)):
                        c[(k // 4) * width + k % 4] = v * step * (-1) ** k
                    add(c, width, type_, scan, set_=set_, cfg=0)
                    add(c[::-1].copy() if width == 4 else c, width, type_, scan, block_type=2, set_=set_, cfg=2)
                    # every level 1: c1 counts up, more than eight of them in a group
                    add(np.full(n, 1.1 * step) * np.where(np.arange(n) % 3 == 0, -1, 1), width, type_, scan, block_type=2, tr_depth=1, set_=set_, cfg=0)
                    add(np.full(n, 2.2 * step), width, type_, scan, set_=set_, cfg=1)
                    # a group of weak coefficients far out: zeroed, or the last position moves in front of it
                    if width > 4:
                        c = np.zeros(n)
                        c[:4] = np.array((5.0, -3.2, 2.1, 1.3)) * step
                        c[width:width + 4] = np.array((2.4, 1.2, -0.9, 0.7)) * step
                        c[(width - 4) * width + width - 4:(width - 4) * width + width] = np.array((0.6, -0.7, 0.55, 0.65)) * step
                        c[4 * width + 4:4 * width + 8] = np.array((0.9, 0.7, -0.8, 0.6)) * step
                        add(c, width, type_, scan, set_=set_, cfg=0)
                        add(c, width, type_, scan, block_type=2, tr_depth=2, set_=set_, cfg=3)
                # sign hiding: two coefficients at a distance of 3 / 4 / 15 in the first group, parities both ways
                for first, last in ((0, 3), (0, 4), (1, 5), (0, 15), (2, 9)):
                    for a, b in ((1.2, 1.3), (2.2, -1.2), (-1.4, 2.3), (-2.45, -3.45), (0.8, 1.6)):
                        step = step_of(width, type_, QPS[24])
                        c = np.zeros(n)
                        c[(first // 4) * width + first % 4] = a * step
                        c[(last // 4) * width + last % 4] = b * step
                        c[width + 1] += 0.45 * step * (-1 if a < 0 else 1)
                        add(c, width, type_, scan, block_type=1 + (first & 1), set_=24, cfg=(0, 2)[last & 1])
    return out


def extra_cases(seed, per_width=300, widths=(4, 8, 16, 32)):
    """further seeded TUs on the fixture's sets, for comparing two implementations directly"""
    g = np.random.default_rng(seed)
    return seeded(g, list(widths), [per_width] * len(widths) if isinstance(per_width, int) else list(per_width))


def pack(cs):
    """the cases as the arrays the fixture stores: coeffs int16 (every TU at a multiple of 4), desc [n, 8] of (offset, width, type,
    scan_mode, block_type, tr_depth, set, cfg)"""
    desc = np.zeros((len(cs), 8), dtype=np.int64)
    at = 0
    for i, (c, width, type_, scan, block_type, tr_depth, set_, cfg) in enumerate(cs):
        desc[i] = (at, width, type_, scan, block_type, tr_depth, set_, cfg)
        at += c.size
    return np.concatenate([c for c, *_ in cs]).astype(np.int16), desc


def unpack(coeffs, desc):
    return [(np.asarray(coeffs[o:o + w * w], dtype=np.int16), int(w), int(t), int(s), int(b), int(d), int(set_), int(cfg))
            for o, w, t, s, b, d, set_, cfg in np.asarray(desc, dtype=np.int64).tolist()]

"""The TUs of tests/golden/coeff_cabac.npz: seeded and directed coefficient blocks over all widths, both types and the allowed scans, with
random context bytes in 0..125 and ranges in 256..510, and magnitudes from +-1 up to +-32767 (and -32768).  cases() builds them; the
counts come from the compiled reference (tests/gen_coeff_cabac_golden.py).  TEST INFRASTRUCTURE.

A case is (coeff int16 [width * width], width, type, scan_mode, tr_skip, set index, configuration index); CONFIGS lists the
(signhide, trskip_enable, lossless) triples, of which the first is the one most TUs use: a call of the batch entry has one."""
import numpy as np

CONFIGS = ((1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1))
N_SETS = 48
SEED = 20240611


def context_sets(seed=SEED):
    """(ranges uint16 [N_SETS], dumps uint8 [N_SETS, 184]): whole context blocks, as a host would dump cabac_data_t.ctx"""
    g = np.random.default_rng(seed)
    dumps = g.integers(0, 126, (N_SETS, 184)).astype(np.uint8)
    ranges = g.integers(256, 511, N_SETS).astype(np.uint16)
    # sets at the edges of the state range: everything at state 0, everything at state 62, and the range's two ends
    dumps[0], dumps[1], dumps[2], dumps[3] = 0, 1, 124, 125
    dumps[4] = g.integers(0, 4, 184)
    dumps[5] = g.integers(120, 126, 184)
    ranges[0], ranges[1], ranges[2], ranges[3] = 256, 510, 256, 510
    return ranges, dumps


def _scans(width):
    return (0, 1, 2) if width <= 8 else (0,)


def cases(seed=SEED):
    g = np.random.default_rng(seed + 1)
    out = []

    def add(c, width, type_, scan, tr_skip=0, set_=None, cfg=0):
        c = np.asarray(c, dtype=np.int16).reshape(width * width)
        out.append((c, width, type_, scan, tr_skip, int(g.integers(0, N_SETS)) if set_ is None else set_, cfg))

    # ---- seeded: density and magnitude classes per width; the large widths are few, they fill the file
    for width, count in ((4, 900), (8, 330), (16, 90), (32, 44)):
        for k in range(count):
            dens = (0.03, 0.1, 0.3, 0.6, 1.0)[k % 5]
            mag = (1, 1, 2, 3, 6, 20, 300, 5000, 32767)[(k // 5) % 9]
            c = g.integers(-mag, mag + 1, width * width) * (g.random(width * width) < dens)
            if k % 11 == 0:                                     # low-pass shaped, as a quantised transform leaves it
                yy, xx = np.divmod(np.arange(width * width), width)
                c = c * (g.random(width * width) < np.exp(-(xx + yy) / (width / 3.0)))
            if not c.any():
                c[int(g.integers(0, width * width))] = 1
            cfg = 0 if k % 6 else 1 + (k // 6) % (len(CONFIGS) - 1)
            add(c, width, (0, 2)[k % 2], _scans(width)[(k // 2) % len(_scans(width))], tr_skip=int(k % 4 == 1), cfg=cfg)
    # ---- directed
    for width in (4, 8, 16, 32):
        n = width * width
        for type_ in (0, 2):
            for scan in _scans(width):
                add(np.zeros(n), width, type_, scan)                                         # nothing to code: 0 bits
                for pos in (0, width - 1, n - width, n - 1, n // 2 + width // 2):            # one coefficient: the corners and the middle
                    for v in (1, -2, 3, -32768, 32767):
                        c = np.zeros(n)
                        c[pos] = v
                        add(c, width, type_, scan, set_=(pos + abs(v)) % 6 if v in (1, 3) else None)
                add(np.full(n, 32767), width, type_, scan)                                   # every escape at its longest
                add(np.full(n, -32768), width, type_, scan)
                add(np.ones(n), width, type_, scan, set_=2)                                  # c1 counts up and stays, every group full
                add(np.ones(n), width, type_, scan, set_=0, cfg=3)
                add(-np.ones(n), width, type_, scan, set_=3)
                for x in range(width):                                                       # the last position in every column and row group
                    c = np.zeros(n)
                    c[(width - 1 - x) * width + x] = 1 + x % 3
                    add(c, width, type_, scan)
                # the Rice parameter climbing in one group, then capped
                c = np.zeros(n)
                c[:4] = (4, 7, 13, 25)
                c[width:width + 4] = (49, 100, 200, 3)
                add(c, width, type_, scan)
                # sign hiding at distance 3 / 4 / 15 in the first group, in every configuration
                for first, last in ((0, 3), (0, 4), (1, 5), (0, 15)):
                    for cfg in range(len(CONFIGS)):
                        c = np.zeros(n)
                        for p in (first, last):
                            c[(p // 4) * width + p % 4] = -1 if p else 2
                        add(c, width, type_, scan, cfg=cfg)
        if width > 4:
            # group patterns: an empty group between full ones, right / lower neighbours alone and together
            for type_ in (0, 2):
                for k in range(12):
                    gmask = g.random((width // 4, width // 4)) < (0.25, 0.5, 0.75)[k % 3]
                    gmask[-1, -1] = k % 2
                    c = g.integers(-3, 4, (width, width)) * np.kron(gmask, np.ones((4, 4), dtype=int))
                    if not c.any():
                        c[0, 0] = 1
                    add(c, width, type_, _scans(width)[k % len(_scans(width))])
    return out


def pack(cs):
    """the cases as the arrays the fixture stores: coeffs int16 (every TU at a multiple of 4), desc [n, 7] int64 of (offset, width, type,
    scan_mode, tr_skip, set, cfg)"""
    desc = np.zeros((len(cs), 7), dtype=np.int64)
    at = 0
    for i, (c, width, type_, scan, tr_skip, set_, cfg) in enumerate(cs):
        desc[i] = (at, width, type_, scan, tr_skip, set_, cfg)
        at += c.size
    return np.concatenate([c for c, *_ in cs]).astype(np.int16), desc

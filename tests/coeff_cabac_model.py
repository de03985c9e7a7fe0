"""A plain model of the reference's CABAC coefficient pricing: what get_coeff_cabac_cost (rdo.c:158-197) returns for one TU, that is the
bits kvz_encode_coeff_nxn (encode_coding_tree.c:49-345) produces in counting mode from a given `range` and context set.  Written from
encode_coding_tree.c, context.c:303-385 and cabac.c:91-282 in plain integers, one bin at a time; it is written from neither the kernel
nor any other restatement.  TEST INFRASTRUCTURE.

The count (23 - bits_left) + 8 * num_buffered_bytes is the number of renormalisation shifts plus the number of bypass bins: every
`bits_left -= n` of cabac.c is matched by `bits_left += 8; num_buffered_bytes++` in kvz_cabac_write, which in counting mode does nothing
else, so `low` never matters.

count_bits() also fills a census: a Counter of the decision classes the TU took, counted once per TU (CLASSES).  MUTANTS are deliberate
errors of the kind a kernel author could make, one at a time (count_bits(..., mutant=name)): the stored cases (tests/coeff_cabac_cases.py)
have to reach every class and to notice every mutant.

`ctx` is the reference's context block, the 184 bytes of cabac_data_t.ctx (cabac.h:53-87), as uc_state values.  Only bytes 32..167, 182
and 183 are read.  The reference indexes cu_sig_model_chroma with 15 + cnt for an 8x8 chroma TU in a horizontal or vertical scan, past
that array's 15 entries into cu_ctx_last_y_luma; the model indexes the flat block, so it does the same."""
import collections

# offsets into cabac_data_t.ctx (cabac.h:53-87)
SIG_CG, SIG_LUMA, SIG_CHROMA = 32, 36, 63
LAST_Y_LUMA, LAST_Y_CHROMA, LAST_X_LUMA, LAST_X_CHROMA = 78, 93, 108, 123
ONE_LUMA, ONE_CHROMA, ABS_LUMA, ABS_CHROMA = 138, 154, 162, 166
TS_LUMA, TS_CHROMA = 182, 183
CTX_BYTES = 184
FIRST_USED, END_USED = 32, 168          # the contiguous part a kvz_hip_coeff_ctx carries in ctx[0..135]

# ITU-T H.265 Tables 9-46 / 9-47 as the reference holds them (cabac.c:28-75)
RANGE_LPS = (
    (128, 176, 208, 240), (128, 167, 197, 227), (128, 158, 187, 216), (123, 150, 178, 205), (116, 142, 169, 195), (111, 135, 160, 185),
    (105, 128, 152, 175), (100, 122, 144, 166), (95, 116, 137, 158), (90, 110, 130, 150), (85, 104, 123, 142), (81, 99, 117, 135),
    (77, 94, 111, 128), (73, 89, 105, 122), (69, 85, 100, 116), (66, 80, 95, 110), (62, 76, 90, 104), (59, 72, 86, 99), (56, 69, 81, 94),
    (53, 65, 77, 89), (51, 62, 73, 85), (48, 59, 69, 80), (46, 56, 66, 76), (43, 53, 63, 72), (41, 50, 59, 69), (39, 48, 56, 65),
    (37, 45, 54, 62), (35, 43, 51, 59), (33, 41, 48, 56), (32, 39, 46, 53), (30, 37, 43, 50), (29, 35, 41, 48), (27, 33, 39, 45),
    (26, 31, 37, 43), (24, 30, 35, 41), (23, 28, 33, 39), (22, 27, 32, 37), (21, 26, 30, 35), (20, 24, 29, 33), (19, 23, 27, 31),
    (18, 22, 26, 30), (17, 21, 25, 28), (16, 20, 23, 27), (15, 19, 22, 25), (14, 18, 21, 24), (14, 17, 20, 23), (13, 16, 19, 22),
    (12, 15, 18, 21), (12, 14, 17, 20), (11, 14, 16, 19), (11, 13, 15, 18), (10, 12, 15, 17), (10, 12, 14, 16), (9, 11, 13, 15),
    (9, 11, 12, 14), (8, 10, 12, 14), (8, 9, 11, 13), (7, 9, 11, 12), (7, 9, 10, 12), (7, 8, 10, 11), (6, 8, 9, 11), (6, 7, 9, 10),
    (6, 7, 8, 9), (2, 2, 2, 2))
NEXT_STATE_LPS = (0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
                  24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63)
RENORM = (6, 5, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2) + (1,) * 16                  # kvz_g_auc_renorm_table
GROUP_IDX = (0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9)   # encoderstate.h:345
MIN_IN_GROUP = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24)
CTX_IND_MAP = (0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8, 8)
SCAN_DIAG, SCAN_HOR, SCAN_VER = 0, 1, 2


def _order(n, mode):
    """positions y * n + x of an n x n square in scan order (tables.c: up-right diagonal, row by row, column by column)"""
    if mode == SCAN_HOR:
        return [y * n + x for y in range(n) for x in range(n)]
    if mode == SCAN_VER:
        return [y * n + x for x in range(n) for y in range(n)]
    return [y * n + (d - y) for d in range(2 * n - 1) for y in range(min(d, n - 1), -1, -1) if d - y < n]


_SCANS = {}


def scan_tables(width, mode):
    """(scan [width * width] of coefficient positions, scan_cg [groups] of group positions): kvz_g_sig_last_scan[mode][log2 - 1] and
    g_sig_last_scan_cg[log2 - 2][mode] (tables.h:37-77).  Modes 1 / 2 exist up to width 8 only."""
    key = (width, mode)
    if key not in _SCANS:
        assert width in (4, 8, 16, 32) and (mode == SCAN_DIAG or (mode in (SCAN_HOR, SCAN_VER) and width <= 8))
        g = width // 4
        cg = _order(g, mode)
        inner = _order(4, mode)
        scan = [((c // g) * 4 + p // 4) * width + (c % g) * 4 + p % 4 for c in cg for p in inner]
        _SCANS[key] = (scan, cg)
    return _SCANS[key]


CLASSES = tuple(
    ["sign:hidden", "sign:not-hidden", "sign:distance-met-but-off"] +
    ["c1:1-to-2", "c1:2-to-3", "c1:stays-3", "c1:to-0", "c1:stays-0"] +
    ["greater2:coded", "greater2:not-coded", "group:more-than-8-non-zeros"] +
    ["rice:%d" % k for k in range(5)] + ["rice:capped-at-4"] +
    ["remain:prefix-le-3", "remain:escape", "remain:none-in-group"] +
    ["last:x-suffix", "last:y-suffix", "last:x-prefix-full", "last:y-prefix-full", "last:vertical-swap"] +
    ["cg:first-inferred", "cg:last-inferred", "cg:coded-1-ctx-0", "cg:coded-1-ctx-1", "cg:coded-0-ctx-0", "cg:coded-0-ctx-1"] +
    ["pattern:%d" % k for k in range(4)] +
    ["sig:dc", "sig:4x4-table", "sig:8x8-diagonal", "sig:8x8-other-scan", "sig:larger-luma", "sig:larger-chroma", "sig:luma-group-offset",
     "sig:chroma-no-group-offset", "sig:inferred", "sig:group-last-coded"] +
    ["ctx-set:bump", "ctx-set:no-bump", "ctx-set:luma-later-group"] +
    ["trskip:bin-0", "trskip:bin-1", "trskip:absent-width", "trskip:absent-disabled"] +
    ["mps:shift", "mps:no-shift"] + ["lps:shift-%d" % k for k in range(1, 7)] +
    ["state:saturates-at-62", "state:mps-flips-at-0", "tu:all-zero"])

# name -> description
MUTANTS = {
    "no-vertical-swap": "the last position's x and y are not swapped for the vertical scan",
    "sign-hide-threshold-3": "a sign is hidden from a distance of 3",
    "sign-hide-ignores-lossless": "a sign is hidden although the TU is coded lossless",
    "c1-not-carried": "c1 restarts at 1 without the ctx_set bump of a group that follows one that ended at 0",
    "c1-counts-to-4": "c1 counts past 3",
    "greater2-always": "the greater-2 flag is coded for every group that has a coefficient",
    "rice-cap-5": "the Rice parameter grows to 5",
    "rice-not-reset": "the Rice parameter is not reset at a group's start",
    "rice-threshold-ge": "the Rice parameter grows at abs >= 3 << r instead of >",
    "escape-at-4": "the remainder's escape starts at prefix 4",
    "base-level-after-8": "base level 2 + first_coeff2 also for the coefficients past the eighth",
    "first-coeff2-at-3": "first_coeff2 falls at abs >= 3 instead of 2",
    "cg-context-right-only": "the group flag's context looks at the right neighbour only",
    "pattern-swapped": "the pattern context's right and lower bits are swapped",
    "sig-inferred-coded": "the flag at a group's last position is coded although it is inferred",
    "sig-dc-from-table": "the DC position takes the table's / the pattern's context instead of 0",
    "sig-8x8-offset-9": "an 8x8 TU takes offset 9 whatever the scan",
    "sig-chroma-group-offset": "the + 3 of a later group also for chroma",
    "sig-chroma-offset-21": "a larger chroma TU takes luma's offset 21",
    "last-luma-shift": "luma's last-position context shift is (index + 3) / 4 without the context offset",
    "last-suffix-rounds-up": "the last position's suffix takes (group index - 1) / 2 bits",
    "last-prefix-no-stop": "the prefix's terminating 0 is also coded at the largest group index",
    "trskip-bin-every-width": "the transform_skip_flag bin is coded at every width",
    "trskip-chroma-luma-context": "a chroma TU's transform_skip_flag takes luma's context",
    "ctx-set-chroma-2": "ctx_set starts at 2 in a chroma TU's later groups",
    "mps-saturates-at-61": "an MPS stops the state at 61",
    "mps-no-flip": "an LPS at state 0 does not flip the MPS",
    "lps-counts-one-bit": "an LPS counts one bit whatever its renormalisation shift",
}


def census_classes():
    return list(CLASSES)


class _Coder:
    def __init__(self, rng, ctx, census, mutant):
        self.range, self.ctx, self.bits, self.census, self.mutant = rng, list(ctx), 0, census, mutant

    def bin(self, index, value):                                # kvz_cabac_encode_bin, cabac.c:91-120
        uc = self.ctx[index]
        state, mps = uc >> 1, uc & 1
        lps = RANGE_LPS[state][(self.range >> 6) & 3]
        self.range -= lps
        if (1 if value else 0) != mps:
            n = RENORM[lps >> 3]
            self.range = lps << n
            self.bits += 1 if self.mutant == "lps-counts-one-bit" else n
            self.census.add("lps:shift-%d" % n)
            if state == 0:
                self.census.add("state:mps-flips-at-0")
                if self.mutant != "mps-no-flip":
                    mps ^= 1
            self.ctx[index] = NEXT_STATE_LPS[state] << 1 | mps
        else:
            if state == 62:
                self.census.add("state:saturates-at-62")
            top = 61 if self.mutant == "mps-saturates-at-61" else 62
            self.ctx[index] = (state + 1 if state < top else state) << 1 | mps
            if self.range >= 256:
                self.census.add("mps:no-shift")
                return
            self.range <<= 1
            self.bits += 1
            self.census.add("mps:shift")

    def ep(self, num_bins):                                     # kvz_cabac_encode_bins_ep: one bit each
        self.bits += num_bins

    def coeff_remain(self, symbol, r):                          # kvz_cabac_write_coeff_remain, cabac.c:263-282
        limit = 4 if self.mutant == "escape-at-4" else 3
        if symbol < (limit << r):
            self.census.add("remain:prefix-le-3")
            self.ep((symbol >> r) + 1)
            self.ep(r)
        else:
            self.census.add("remain:escape")
            length = r
            symbol -= limit << r
            while symbol >= (1 << length):
                symbol -= 1 << length
                length += 1
            self.ep(limit + length + 1 - r)
            self.ep(length)


def _last_xy(cod, x, y, width, type_, scan_mode):               # encode_last_significant_xy, encode_coding_tree.c:49-101
    index = width.bit_length() - 3
    ctx_offset = 0 if type_ else index * 3 + (index + 1) // 4
    shift = index if type_ else (index + 3) // 4
    if cod.mutant == "last-luma-shift" and not type_:
        ctx_offset = 0
    base_x = LAST_X_CHROMA if type_ else LAST_X_LUMA
    base_y = LAST_Y_CHROMA if type_ else LAST_Y_LUMA
    if scan_mode == SCAN_VER:
        cod.census.add("last:vertical-swap")
        if cod.mutant != "no-vertical-swap":
            x, y = y, x
    gx, gy = GROUP_IDX[x], GROUP_IDX[y]
    top = GROUP_IDX[width - 1]
    for base, g, name in ((base_x, gx, "x"), (base_y, gy, "y")):
        for k in range(g):
            cod.bin(base + ctx_offset + (k >> shift), 1)
        if g < top or (cod.mutant == "last-prefix-no-stop" and top < 9):
            cod.bin(base + ctx_offset + (g >> shift), 0)
        if g >= top:
            cod.census.add("last:%s-prefix-full" % name)
    less = 1 if cod.mutant == "last-suffix-rounds-up" else 2
    if gx > 3:
        cod.census.add("last:x-suffix")
        cod.ep((gx - less) // 2)
    if gy > 3:
        cod.census.add("last:y-suffix")
        cod.ep((gy - less) // 2)


def _sig_ctx_inc(cod, pattern, scan_mode, x, y, log2, type_):   # kvz_context_get_sig_ctx_inc, context.c:354-385
    if x + y == 0 and cod.mutant != "sig-dc-from-table":
        cod.census.add("sig:dc")
        return 0
    if log2 == 2:
        cod.census.add("sig:4x4-table")
        return CTX_IND_MAP[4 * y + x]
    if log2 == 3:
        cod.census.add("sig:8x8-diagonal" if scan_mode == SCAN_DIAG else "sig:8x8-other-scan")
        offset = 9 if scan_mode == SCAN_DIAG or cod.mutant == "sig-8x8-offset-9" else 15
    else:
        cod.census.add("sig:larger-chroma" if type_ else "sig:larger-luma")
        offset = 21 if type_ == 0 or cod.mutant == "sig-chroma-offset-21" else 12
    xs, ys = x & 3, y & 3
    if pattern == 0:
        cnt = (2 if xs + ys == 0 else 1) if xs + ys <= 2 else 0
    elif pattern == 1:
        cnt = (2 if ys == 0 else 1) if ys <= 1 else 0
    elif pattern == 2:
        cnt = (2 if xs == 0 else 1) if xs <= 1 else 0
    else:
        cnt = 2
    later = (x >> 2) + (y >> 2) > 0
    if later:
        cod.census.add("sig:chroma-no-group-offset" if type_ else "sig:luma-group-offset")
    return (3 if later and (type_ == 0 or cod.mutant == "sig-chroma-group-offset") else 0) + offset + cnt


def count_bits(coeff, width, type_, scan_mode, tr_skip, rng, ctx, signhide=1, trskip_enable=1, lossless=0, mutant=None, census=None):
    """bits of one TU.  coeff: width * width integers, row-major; type_ 0 (luma) / 2 (chroma); ctx: 184 uc_state values, not written."""
    assert mutant is None or mutant in MUTANTS
    assert len(ctx) == CTX_BYTES and type_ in (0, 2) and len(coeff) == width * width
    seen = set()
    try:
        return _count(list(int(c) for c in coeff), width, type_, scan_mode, tr_skip, rng, ctx, signhide, trskip_enable, lossless, mutant, seen)
    finally:
        if census is not None:
            census.update(seen)


def _count(coeff, width, type_, scan_mode, tr_skip, rng, ctx, signhide, trskip_enable, lossless, mutant, census):
    if not any(coeff):                                           # rdo.c:165-173
        census.add("tu:all-zero")
        return 0
    cod = _Coder(rng, ctx, census, mutant)
    log2 = width.bit_length() - 1
    g = width >> 2
    scan, scan_cg = scan_tables(width, scan_mode)
    sig_cg = [0] * (g * g)
    for cy in range(g):
        for cx in range(g):
            if any(coeff[(cy * 4 + r) * width + cx * 4 + c] for r in range(4) for c in range(4)):
                sig_cg[cx + cy * g] = 1
    scan_cg_last = g * g - 1
    while not sig_cg[scan_cg[scan_cg_last]]:
        scan_cg_last -= 1
    scan_pos_last = scan_cg_last * 16 + 15
    while not coeff[scan[scan_pos_last]]:
        scan_pos_last -= 1
    pos_last = scan[scan_pos_last]

    if (width == 4 or mutant == "trskip-bin-every-width") and trskip_enable:
        census.add("trskip:bin-1" if tr_skip else "trskip:bin-0")
        cod.bin(TS_LUMA if type_ == 0 or mutant == "trskip-chroma-luma-context" else TS_CHROMA, tr_skip)
    else:
        census.add("trskip:absent-width" if trskip_enable else "trskip:absent-disabled")
    _last_xy(cod, pos_last & (width - 1), pos_last >> log2, width, type_, scan_mode)

    base_sig = SIG_LUMA if type_ == 0 else SIG_CHROMA
    c1 = 1
    rice = 0
    scan_pos_sig = scan_pos_last
    for i in range(scan_cg_last, -1, -1):
        sub_pos = i << 4
        cg_blk_pos = scan_cg[i]
        cg_y, cg_x = divmod(cg_blk_pos, g)
        absc, signs, n_signs = [], 0, 0
        last_nz, first_nz = -1, 16
        if mutant != "rice-not-reset":
            rice = 0
        if scan_pos_sig == scan_pos_last:
            absc.append(abs(coeff[pos_last]))
            signs = 1 if coeff[pos_last] < 0 else 0
            last_nz = first_nz = scan_pos_sig
            scan_pos_sig -= 1
        right = 1 if cg_x < g - 1 and sig_cg[cg_y * g + cg_x + 1] else 0
        lower = 1 if cg_y < g - 1 and sig_cg[(cg_y + 1) * g + cg_x] else 0
        if i == scan_cg_last or i == 0:
            census.add("cg:last-inferred" if i == scan_cg_last else "cg:first-inferred")
            sig_cg[cg_blk_pos] = 1
        else:
            c = right if mutant == "cg-context-right-only" else (right | lower)     # kvz_context_get_sig_coeff_group, context.c:303-315
            census.add("cg:coded-%d-ctx-%d" % (sig_cg[cg_blk_pos], right | lower))
            cod.bin(SIG_CG + type_ + c, sig_cg[cg_blk_pos])
        if sig_cg[cg_blk_pos]:
            pattern = -1 if width == 4 else right + (lower << 1)                    # kvz_context_calc_pattern_sig_ctx, context.c:327-339
            if width != 4:
                census.add("pattern:%d" % pattern)
                if mutant == "pattern-swapped":
                    pattern = lower + (right << 1)
            while scan_pos_sig >= sub_pos:
                blk_pos = scan[scan_pos_sig]
                y, x = blk_pos >> log2, blk_pos & (width - 1)
                sig = 1 if coeff[blk_pos] else 0
                if scan_pos_sig > sub_pos or i == 0 or absc:
                    if scan_pos_sig == sub_pos and i != 0:
                        census.add("sig:group-last-coded")
                    cod.bin(base_sig + _sig_ctx_inc(cod, pattern, scan_mode, x, y, log2, type_), sig)
                else:
                    census.add("sig:inferred")
                    if mutant == "sig-inferred-coded":
                        cod.bin(base_sig + _sig_ctx_inc(cod, pattern, scan_mode, x, y, log2, type_), sig)
                if sig:
                    absc.append(abs(coeff[blk_pos]))
                    signs = 2 * signs + (1 if coeff[blk_pos] < 0 else 0)
                    if last_nz == -1:
                        last_nz = scan_pos_sig
                    first_nz = scan_pos_sig
                scan_pos_sig -= 1
        else:
            scan_pos_sig = sub_pos - 1
        if not absc:
            continue
        nnz = len(absc)
        distance = 3 if mutant == "sign-hide-threshold-3" else 4
        far = last_nz - first_nz >= distance
        hidden = far and (not lossless or mutant == "sign-hide-ignores-lossless")
        ctx_set = 2 if i > 0 and (type_ == 0 or mutant == "ctx-set-chroma-2") else 0
        if i > 0 and type_ == 0:
            census.add("ctx-set:luma-later-group")
        if c1 == 0:
            census.add("ctx-set:bump")
            if mutant != "c1-not-carried":
                ctx_set += 1
        else:
            census.add("ctx-set:no-bump")
        c1 = 1
        base_one = (ONE_LUMA if type_ == 0 else ONE_CHROMA) + 4 * ctx_set
        first_c2 = -1
        if nnz > 8:
            census.add("group:more-than-8-non-zeros")
        for idx in range(min(nnz, 8)):
            symbol = 1 if absc[idx] > 1 else 0
            cod.bin(base_one + c1, symbol)
            if symbol:
                census.add("c1:stays-0" if c1 == 0 else "c1:to-0")
                c1 = 0
                if first_c2 == -1:
                    first_c2 = idx
            elif 0 < c1 < (4 if mutant == "c1-counts-to-4" else 3):
                census.add("c1:%d-to-%d" % (c1, c1 + 1))
                c1 += 1
            elif c1 == 3:
                census.add("c1:stays-3")
        if c1 == 0 or mutant == "greater2-always":
            if first_c2 != -1 or mutant == "greater2-always":
                k = first_c2 if first_c2 != -1 else 0
                census.add("greater2:coded")
                cod.bin((ABS_LUMA if type_ == 0 else ABS_CHROMA) + ctx_set, 1 if absc[k] > 2 else 0)
        else:
            census.add("greater2:not-coded")
        if signhide and hidden:
            census.add("sign:hidden")
            cod.ep(nnz - 1)
        else:
            census.add("sign:distance-met-but-off" if far else "sign:not-hidden")
            cod.ep(nnz)
        if c1 == 0 or nnz > 8:
            first_coeff2 = 1
            coded = False
            for idx in range(nnz):
                base_level = 2 + first_coeff2 if idx < 8 or mutant == "base-level-after-8" else 1
                if absc[idx] >= base_level:
                    coded = True
                    census.add("rice:%d" % rice)
                    cod.coeff_remain(absc[idx] - base_level, rice)
                    grows = absc[idx] >= 3 << rice if mutant == "rice-threshold-ge" else absc[idx] > 3 << rice
                    if grows:
                        if rice == 4:
                            census.add("rice:capped-at-4")
                        rice = min(rice + 1, 5 if mutant == "rice-cap-5" else 4)
                if absc[idx] >= (3 if mutant == "first-coeff2-at-3" else 2):
                    first_coeff2 = 0
            if not coded:
                census.add("remain:none-in-group")
        else:
            census.add("remain:none-in-group")
    return cod.bits

"""A plain model of the reference's rate-distortion optimised quantisation: what kvz_rdoq (rdo.c:548-881) leaves in dest_coeff for one
TU, with kvz_get_ic_rate (:233-278), kvz_get_coded_level (:297-339), get_rate_last / calc_last_bits (:350-395) and kvz_rdoq_sign_hiding
(:405-539).  Written from rdo.c and context.c:303-385 in Python integers and floats: a Python float is an IEEE binary64 value and
Python never fuses a multiplication with an addition, which is what the reference's object code does as well.  It is written from
neither the kernel nor any other restatement.  Bit depth 8.  TEST INFRASTRUCTURE.

rdoq() also fills a census: a Counter of the decision classes the TU took, counted once per TU (CLASSES).  MUTANTS are deliberate errors
of the kind a kernel author could make, one at a time (rdoq(..., mutant=name)): the stored cases (tests/rdoq_cases.py) have to reach every
class and to notice every mutant.  No mutant fuses a multiplication with an addition: a contraction moves a cost by one unit in the last
place, which changes a decision only where two costs tie to that precision, and no TU of the fixture does (tried); the kernel's build
switches contraction off instead (tests/test_rdoq_abi.py looks at both switches).  Three more errors cannot show either and are
not listed: a chroma TU that takes luma's list (the default lists of the three colours are equal), sign hiding that ignores abs_sum >= 2
(a TU below that holds at most one level, so no group reaches the distance of 4), and an rd_factor without its + 0.5 (it moves a price by
one part in thousands at the lambdas an encoder uses).

Every array the reference leaves uninitialised on its stack (cost_coeff, cost_sig, cost_coeff0, cost_coeffgroup_sig, sh_rates, the last-
position bits, dest_coeff) starts out filled with UNWRITTEN here, an object that raises UnwrittenRead on every use as a number -- arithmetic,
comparison, conversion and the truth test of `if dest[blkpos]:` alike -- so an entry that was never written cannot pass for a value.
rdoq(..., forget=name) leaves one write out on purpose (FORGETTABLE), which is how the tests show that the poison bites.

`ctx` is the reference's context block, the 184 bytes of cabac_data_t.ctx (cabac.h:53-87), as uc_state values.  `quant` and `err_scale`
are the packed tables of kvz_hip_rdoq_tables (include/kvz_hip.h): the model picks the TU's table itself."""
import collections

from coeff_cabac_model import (ABS_CHROMA, ABS_LUMA, CTX_BYTES, CTX_IND_MAP, GROUP_IDX, LAST_X_CHROMA, LAST_X_LUMA, LAST_Y_CHROMA, LAST_Y_LUMA,
                               ONE_CHROMA, ONE_LUMA, SCAN_DIAG, SCAN_VER, SIG_CG, SIG_CHROMA, SIG_LUMA, scan_tables)

QT_CBF_LUMA, QT_CBF_CHROMA, ROOT_CBF = 16, 20, 181          # offsets into cabac_data_t.ctx (cabac.h:61-62, :84)
CU_INTRA, CU_INTER = 1, 2                                    # cu.h:39-41
FRAC_BITS = 15                                               # CTX_FRAC_BITS, rdo.h:65
ONE_BIT = 1 << FRAC_BITS
C1FLAG_NUMBER, C2FLAG_NUMBER, SBH_THRESHOLD = 8, 1, 4        # encoderstate.h:355-356, global.h
MAX_DOUBLE = 1.7e+308                                        # global.h:269
MAX_INT, MAX_INT64 = 0x7fffffff, 0x7fffffffffffffff
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)                  # kvz_g_inv_quant_scales, scalinglist.c:67
CHROMA_SCALE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32,
                33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51)   # kvz_g_chroma_scale, transform.c:44-50
SL_TABLE_LEN = 48960

# the price of a bin in 1 / 32768 bit, indexed uc_state ^ bin (HM's table; kvz_entropy_bits, rdo.c:53-63)
ENTROPY_BITS = (
    0x08000, 0x08000, 0x076da, 0x089a0, 0x06e92, 0x09340, 0x0670a, 0x09cdf, 0x06029, 0x0a67f, 0x059dd, 0x0b01f, 0x05413, 0x0b9bf, 0x04ebf, 0x0c35f,
    0x049d3, 0x0ccff, 0x04546, 0x0d69e, 0x0410d, 0x0e03e, 0x03d22, 0x0e9de, 0x0397d, 0x0f37e, 0x03619, 0x0fd1e, 0x032ee, 0x106be, 0x02ffa, 0x1105d,
    0x02d37, 0x119fd, 0x02aa2, 0x1239d, 0x02836, 0x12d3d, 0x025f2, 0x136dd, 0x023d1, 0x1407c, 0x021d2, 0x14a1c, 0x01ff2, 0x153bc, 0x01e2f, 0x15d5c,
    0x01c87, 0x166fc, 0x01af7, 0x1709b, 0x0197f, 0x17a3b, 0x0181d, 0x183db, 0x016d0, 0x18d7b, 0x01595, 0x1971b, 0x0146c, 0x1a0bb, 0x01354, 0x1aa5a,
    0x0124c, 0x1b3fa, 0x01153, 0x1bd9a, 0x01067, 0x1c73a, 0x00f89, 0x1d0da, 0x00eb7, 0x1da79, 0x00df0, 0x1e419, 0x00d34, 0x1edb9, 0x00c82, 0x1f759,
    0x00bda, 0x200f9, 0x00b3c, 0x20a99, 0x00aa5, 0x21438, 0x00a17, 0x21dd8, 0x00990, 0x22778, 0x00911, 0x23118, 0x00898, 0x23ab8, 0x00826, 0x24458,
    0x007ba, 0x24df7, 0x00753, 0x25797, 0x006f2, 0x26137, 0x00696, 0x26ad7, 0x0063f, 0x27477, 0x005ed, 0x27e17, 0x0059f, 0x287b6, 0x00554, 0x29156,
    0x0050e, 0x29af6, 0x004cc, 0x2a497, 0x0048d, 0x2ae35, 0x00451, 0x2b7d6, 0x00418, 0x2c176, 0x003e2, 0x2cb15, 0x003af, 0x2d4b5, 0x0037f, 0x2de55)

CLASSES = tuple(
    ["tu:all-zero", "max:0", "max:1-2", "max:ge-3", "pos:last", "pos:not-last", "level:below-max", "level:zero-from-nonzero-max"] +
    ["rate:remain-prefix", "rate:remain-escape", "rate:escape-loop", "rate:level-1", "rate:level-2", "rate:level-0", "rate:greater1-in-remain",
     "rate:greater2-in-remain", "rate:base-level-1", "rate:base-level-2", "rate:base-level-3"] +
    ["rice:raised", "rice:capped-at-4", "c1-idx:ge-8", "c2-idx:ge-1"] + ["ctx-set:%d" % k for k in range(4)] +
    ["cg:found-empty", "cg:zeroed", "cg:kept", "cg:nnz-before-pos0-is-0", "cbf:root", "cbf:qt-luma-depth-0", "cbf:qt-luma-deeper", "cbf:qt-chroma"] +
    ["last:found-last", "last:moved", "last:kept", "last:tu-emptied", "last:vertical-swap", "last:x-suffix", "last:y-suffix"] +
    ["sh:off", "sh:abs-sum-below-2", "sh:skip-by-threshold", "sh:parity-right", "sh:increment", "sh:decrement", "sh:zero-to-one",
     "sh:first-nonzero-guard", "sh:sign-guard", "sh:last-coefficient-minus-4-bits", "sh:one-to-zero"])

MUTANTS = {
    "no-vertical-swap": "get_rate_last takes x and y unswapped for the vertical scan",
    "rice-cap-5": "the Rice parameter grows to 5",
    "rice-threshold-ge": "the Rice parameter grows at level >= 3 << r instead of >",
    "only-max-level": "kvz_get_coded_level tries max_abs_level alone, not the level below",
    "no-group-zeroing": "a coefficient group is never zeroed (rdo.c:790-807)",
    "no-last-search": "the last position stays where the first loop found it",
    "found-last-ignored": "the last-position search walks on past a level above 1",
    "root-cbf-ignored": "an inter luma TU takes the qt-cbf branch",
    "luma-cbf-by-depth": "the luma qt-cbf context is tr_depth instead of !tr_depth",
    "ctx-set-no-bump": "ctx_set is not raised after a group that ended with c1 == 0",
    "c1-idx-no-limit": "the base level ignores c1_idx >= 8",
    "c2-idx-no-limit": "the base level ignores c2_idx >= 1",
    "nnz-before-pos0-ignored": "sig_cost_0 is never taken out of a group's sig cost",
    "cost-sig-of-zero-levels-kept": "the search does not subtract cost_sig of a zero level (rdo.c:859)",
    "err-scale-of-dc": "every coefficient takes the error scale of position 0",
    "inter-takes-intra-list": "block_type does not select the list",
    "chroma-qp-unscaled": "a chroma TU takes state->qp without kvz_get_scaled_qp",
    "sh-threshold-3": "sign hiding runs from a distance of 3",
    "sh-no-first-nonzero-guard": "sign hiding may turn a group's first non-zero coefficient into zero",
    "sh-no-sign-guard": "sign hiding may raise a zero in front of the first non-zero against the sign",
    "sh-no-last-bonus": "the -4 bits of the last coefficient are left out",
}


def scaled_qp(type_, qp):                                      # kvz_get_scaled_qp, transform.c:129-143, qp_offset 0
    return qp if type_ == 0 else CHROMA_SCALE[min(max(qp, 0), 57)]


def table_offset(size_id, list_id, rem):
    return 36 * (0, 16, 80, 336)[size_id] + (6 * list_id + rem) * (16 << (2 * size_id))


def _i16(v):
    return ((v + 32768) & 0xffff) - 32768


class UnwrittenRead(Exception):
    """an array entry was used before anything was written to it"""


class _Unwritten:
    def _raise(self, *args):
        raise UnwrittenRead("an entry that was never written is read")
    __bool__ = __int__ = __float__ = __index__ = __neg__ = __abs__ = _raise
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __rshift__ = __lshift__ = __and__ = __rand__ = _raise
    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _raise
    __hash__ = None

    def __repr__(self):
        return "UNWRITTEN"


UNWRITTEN = _Unwritten()
# writes rdoq(..., forget=name) leaves out, each at the last scan position: every one of them is read later on every TU that holds a level
FORGETTABLE = ("cost_coeff", "cost_sig", "cost_coeff0", "dest", "last_x_bits", "cost_coeffgroup_sig")


class _Tu:
    pass


def _bits(t, index, bin_):                                      # CTX_ENTROPY_BITS, rdo.h:70
    return ENTROPY_BITS[(t.ctx[index] ^ bin_) & 127]          # the reference's bytes are 0..125; the entry reads any other as byte & 127


def _ic_rate(t, abs_level, one_i, abs_i, rice, c1_idx, c2_idx, count=True):     # kvz_get_ic_rate, rdo.c:233-278
    add = t.census.add if count else (lambda name: None)
    rate = ONE_BIT
    if c1_idx < C1FLAG_NUMBER or t.mutant == "c1-idx-no-limit":
        base_level = 2 + (1 if c2_idx < C2FLAG_NUMBER or t.mutant == "c2-idx-no-limit" else 0)
    else:
        base_level = 1
    if abs_level >= base_level:
        add("rate:base-level-%d" % base_level)
        symbol = abs_level - base_level
        if symbol < (3 << rice):
            add("rate:remain-prefix")
            length = symbol >> rice
            rate += (length + 1 + rice) * ONE_BIT
        else:
            add("rate:remain-escape")
            length = rice
            symbol -= 3 << rice
            while symbol >= (1 << length):
                add("rate:escape-loop")
                symbol -= 1 << length
                length += 1
            rate += (3 + length + 1 - rice + length) * ONE_BIT
        if c1_idx < C1FLAG_NUMBER:
            add("rate:greater1-in-remain")
            rate += _bits(t, one_i, 1)
            if c2_idx < C2FLAG_NUMBER:
                add("rate:greater2-in-remain")
                rate += _bits(t, abs_i, 1)
    elif abs_level == 1:
        add("rate:level-1")
        rate += _bits(t, one_i, 0)
    elif abs_level == 2:
        add("rate:level-2")
        rate += _bits(t, one_i, 1)
        rate += _bits(t, abs_i, 0)
    else:
        add("rate:level-0")
    return rate


def _coded_level(t, scanpos, level_double, max_abs_level, sig_i, one_i, abs_i, rice, c1_idx, c2_idx, temp, last):
    """kvz_get_coded_level, rdo.c:297-339; writes cost_coeff[scanpos] and cost_sig[scanpos], reads cost_coeff0[scanpos]"""
    lam = t.lam
    cur_cost_sig = 0.0
    best = 0
    if not last and max_abs_level < 3:
        t.cost_sig[scanpos] = lam * _bits(t, sig_i, 0)
        t.cost_coeff[scanpos] = t.cost_coeff0[scanpos] + t.cost_sig[scanpos]
        if max_abs_level == 0:
            return best
    else:
        t.cost_coeff[scanpos] = MAX_DOUBLE
    if not last:
        cur_cost_sig = lam * _bits(t, sig_i, 1)
    min_abs_level = max_abs_level - 1 if max_abs_level > 1 else 1
    if t.mutant == "only-max-level":
        min_abs_level = max_abs_level
    for abs_level in range(max_abs_level, min_abs_level - 1, -1):
        err = float(level_double - abs_level * (1 << t.q_bits))
        rate = _ic_rate(t, abs_level, one_i, abs_i, rice, c1_idx, c2_idx)
        cur_cost = err * err * temp + lam * rate
        cur_cost += cur_cost_sig
        if cur_cost < t.cost_coeff[scanpos]:
            best = abs_level
            t.cost_coeff[scanpos] = cur_cost
            t.cost_sig[scanpos] = cur_cost_sig
    return best


def _sig_ctx_inc(pattern, scan_mode, x, y, log2, type_):        # kvz_context_get_sig_ctx_inc, context.c:354-385
    if x + y == 0:
        return 0
    if log2 == 2:
        return CTX_IND_MAP[4 * y + x]
    offset = (9 if scan_mode == SCAN_DIAG else 15) if log2 == 3 else (21 if type_ == 0 else 12)
    xs, ys = x & 3, y & 3
    if pattern == 0:
        cnt = (2 if xs + ys == 0 else 1) if xs + ys <= 2 else 0
    elif pattern == 1:
        cnt = (2 if ys == 0 else 1) if ys <= 1 else 0
    elif pattern == 2:
        cnt = (2 if xs == 0 else 1) if xs <= 1 else 0
    else:
        cnt = 2
    return (3 if type_ == 0 and (x >> 2) + (y >> 2) > 0 else 0) + offset + cnt


def _neighbours(flags, x, y, g):
    right = 1 if x < g - 1 and flags[y * g + x + 1] else 0
    lower = 1 if y < g - 1 and flags[(y + 1) * g + x] else 0
    return right, lower


def _rate_last(t, pos_x, pos_y):                                # get_rate_last, rdo.c:350-364
    ctx_x, ctx_y = GROUP_IDX[pos_x], GROUP_IDX[pos_y]
    cost = float(t.last_x_bits[ctx_x] + t.last_y_bits[ctx_y])
    if ctx_x > 3:
        t.census.add("last:x-suffix")
        cost += ONE_BIT * ((ctx_x - 2) >> 1)
    if ctx_y > 3:
        t.census.add("last:y-suffix")
        cost += ONE_BIT * ((ctx_y - 2) >> 1)
    return t.lam * cost


def _calc_last_bits(t, width, type_):                           # rdo.c:366-395
    index = width.bit_length() - 3
    offset = 0 if type_ else index * 3 + ((index + 1) >> 2)
    shift = index if type_ else (index + 3) >> 2
    top = GROUP_IDX[width - 1]
    for name, base in (("last_x_bits", LAST_X_CHROMA if type_ else LAST_X_LUMA), ("last_y_bits", LAST_Y_CHROMA if type_ else LAST_Y_LUMA)):
        out, bits = [UNWRITTEN] * 32, 0
        for c in range(top):
            out[c] = bits + _bits(t, base + offset + (c >> shift), 0)
            bits += _bits(t, base + offset + (c >> shift), 1)
        out[top] = bits
        setattr(t, name, out)


def _sign_hiding(t, qp_scaled, scan, last_pos, coeffs, q):      # kvz_rdoq_sign_hiding, rdo.c:405-539
    add = t.census.add
    inv_quant = INV_QUANT_SCALES[qp_scaled % 6]
    rd_factor = int(inv_quant * inv_quant * (1 << (2 * (qp_scaled // 6))) / t.lam / 16 / 1 + 0.5)
    last_cg = (last_pos - 1) >> 4
    threshold = 3 if t.mutant == "sh-threshold-3" else SBH_THRESHOLD
    for cg_scan in range(last_cg, -1, -1):
        at = cg_scan << 4
        last_nz = -1
        for i in range(15, -1, -1):
            if q[scan[i + at]]:
                last_nz = i
                break
        first_nz = 16
        for i in range(0, last_nz + 1):
            if q[scan[i + at]]:
                first_nz = i
                break
        if last_nz - first_nz < threshold:
            add("sh:skip-by-threshold")
            continue
        signbit = 1 if q[scan[at + first_nz]] <= 0 else 0
        abs_sum = sum(q[scan[i + at]] for i in range(first_nz, last_nz + 1))
        if signbit == (abs_sum & 1):
            add("sh:parity-right")
            continue
        best = (MAX_INT64, 0, 0, None)
        last_coeff_scan = last_nz if cg_scan == last_cg else 15
        for coeff_scan in range(last_coeff_scan, -1, -1):
            pos = scan[coeff_scan + at]
            quant_cost_in_bits = rd_factor * t.quant_delta[pos]
            abs_coeff = abs(q[pos])
            tag = None
            if abs_coeff != 0:
                inc_bits, dec_bits = t.inc[pos], t.dec[pos]
                if abs_coeff == 1:
                    dec_bits -= ONE_BIT + t.sig_coeff_inc[pos]
                if cg_scan == last_cg and last_nz == coeff_scan and abs_coeff == 1 and t.mutant != "sh-no-last-bonus":
                    dec_bits -= 4 * ONE_BIT
                    tag = "sh:last-coefficient-minus-4-bits"
                inc_bits = -quant_cost_in_bits + inc_bits
                dec_bits = quant_cost_in_bits + dec_bits
                if inc_bits < dec_bits:
                    change, cost, tag = 1, inc_bits, None
                else:
                    change, cost = -1, dec_bits
                    if coeff_scan == first_nz and abs_coeff == 1:
                        add("sh:first-nonzero-guard")
                        if t.mutant != "sh-no-first-nonzero-guard":
                            cost = MAX_INT64
                kind = "sh:increment" if change == 1 else ("sh:one-to-zero" if abs_coeff == 1 else "sh:decrement")
            else:
                bits = ONE_BIT + t.inc[pos] + t.sig_coeff_inc[pos]
                cost = -abs(quant_cost_in_bits) + bits
                change, kind = 1, "sh:zero-to-one"
                if coeff_scan < first_nz and (0 if coeffs[pos] >= 0 else 1) != signbit:
                    add("sh:sign-guard")
                    if t.mutant != "sh-no-sign-guard":
                        cost = MAX_INT64
            if cost < best[0]:
                best = (cost, pos, change, (kind, tag))
        cost, pos, change, tags = best
        if tags is not None:
            add(tags[0])
            if tags[0] == "sh:one-to-zero":
                add("sh:decrement")
                if tags[1]:
                    add(tags[1])
        if q[pos] == 32767 or q[pos] == -32768:
            change = -1
        q[pos] = _i16(q[pos] + change if coeffs[pos] >= 0 else q[pos] - change)


def rdoq(coef, width, type_, scan_mode, block_type, tr_depth, qp, lam, ctx, quant, err_scale, signhide=1, mutant=None, census=None, forget=None):
    """dest_coeff of one TU: width * width integers.  coef: width * width integers, row-major; type_ 0 (luma) / 2 (chroma); block_type
    CU_INTRA / CU_INTER; ctx: 184 uc_state values; quant / err_scale: the packed tables (SL_TABLE_LEN values each)."""
    assert mutant is None or mutant in MUTANTS
    assert forget is None or forget in FORGETTABLE
    assert len(ctx) == CTX_BYTES and type_ in (0, 2) and len(coef) == width * width and block_type in (CU_INTRA, CU_INTER)
    seen = set()
    try:
        return _rdoq([int(c) for c in coef], width, type_, scan_mode, block_type, tr_depth, int(qp), float(lam), [int(c) for c in ctx], quant, err_scale,
                     signhide, mutant, seen, forget)
    finally:
        if census is not None:
            census.update(seen)


def _rdoq(coef, width, type_, scan_mode, block_type, tr_depth, qp, lam, ctx, quant, err_scale, signhide, mutant, census, forget=None):
    t = _Tu()
    t.ctx, t.census, t.mutant = ctx, census, mutant
    t.lam = lam
    add = census.add
    n = width * width
    log2 = width.bit_length() - 1
    g = width >> 2
    qp_scaled = qp if mutant == "chroma-qp-unscaled" else scaled_qp(type_, qp)
    t.q_bits = q_bits = 14 + qp_scaled // 6 + (15 - 8 - log2)
    list_id = (0 if block_type == CU_INTRA or mutant == "inter-takes-intra-list" else 3) + (1 if type_ else 0)
    at = table_offset(log2 - 2, list_id, qp_scaled % 6)
    quant_coeff = [int(v) for v in quant[at:at + n]]
    err = [float(v) for v in err_scale[at:at + n]]
    if mutant == "err-scale-of-dc":
        err = [err[0]] * n
    scan, scan_cg = scan_tables(width, scan_mode)
    dest = [UNWRITTEN] * n
    t.cost_coeff, t.cost_sig, t.cost_coeff0 = [UNWRITTEN] * n, [UNWRITTEN] * n, [UNWRITTEN] * n
    t.inc, t.dec, t.sig_coeff_inc, t.quant_delta = [UNWRITTEN] * n, [UNWRITTEN] * n, [UNWRITTEN] * n, [UNWRITTEN] * n
    cg_num = n >> 4
    cost_coeffgroup_sig = [UNWRITTEN] * 64
    sig_coeffgroup_flag = [0] * cg_num
    half = 1 << (q_bits - 1)

    def level_of(blkpos):
        level_double = min(abs(coef[blkpos]) * quant_coeff[blkpos], MAX_INT - half)      # a 64-bit product, then the clamp of rdo.c:629
        return level_double, (level_double + half) >> q_bits

    # ===== the last coefficient group and scan position, rdo.c:619-646
    last_scanpos = cg_last_scanpos = -1
    ctx_set = 0
    for cg_scanpos in range(cg_num - 1, -1, -1):
        for scanpos_in_cg in range(15, -1, -1):
            scanpos = cg_scanpos * 16 + scanpos_in_cg
            blkpos = scan[scanpos]
            if level_of(blkpos)[1] > 0:
                last_scanpos = scanpos
                ctx_set = 2 if scanpos > 0 and type_ == 0 else 0
                cg_last_scanpos = cg_scanpos
                t.sig_coeff_inc[blkpos] = 0
                break
            dest[blkpos] = 0
        if last_scanpos != -1:
            break
    if last_scanpos == -1:
        add("tu:all-zero")
        return dest
    for cg_scanpos in range(cg_last_scanpos, -1, -1):
        cost_coeffgroup_sig[cg_scanpos] = 0.0
    _calc_last_bits(t, width, type_)
    if forget == "cost_coeffgroup_sig":
        cost_coeffgroup_sig[cg_last_scanpos] = UNWRITTEN
    if forget == "last_x_bits":
        t.last_x_bits = [UNWRITTEN] * 32

    base_sig = SIG_LUMA if type_ == 0 else SIG_CHROMA
    base_one = ONE_LUMA if type_ == 0 else ONE_CHROMA
    base_abs = ABS_LUMA if type_ == 0 else ABS_CHROMA
    c1, c2, rice, c1_idx, c2_idx = 1, 0, 0, 0, 0
    base_cost = block_uncoded_cost = 0.0
    for cg_scanpos in range(cg_last_scanpos, -1, -1):
        cg_blkpos = scan_cg[cg_scanpos]
        cg_pos_y, cg_pos_x = divmod(cg_blkpos, g)
        right, lower = _neighbours(sig_coeffgroup_flag, cg_pos_x, cg_pos_y, g)
        pattern = -1 if width == 4 else right + (lower << 1)
        coded_level_and_dist = uncoded_dist = sig_cost = sig_cost_0 = 0.0
        nnz_before_pos0 = 0
        for scanpos_in_cg in range(15, -1, -1):
            scanpos = cg_scanpos * 16 + scanpos_in_cg
            if scanpos > last_scanpos:
                continue
            blkpos = scan[scanpos]
            temp = err[blkpos]
            level_double, max_abs_level = level_of(blkpos)
            add("max:0" if max_abs_level == 0 else "max:1-2" if max_abs_level < 3 else "max:ge-3")
            e = float(level_double)
            t.cost_coeff0[scanpos] = e * e * temp
            if forget == "cost_coeff0" and scanpos == last_scanpos:
                t.cost_coeff0[scanpos] = UNWRITTEN
            block_uncoded_cost += t.cost_coeff0[scanpos]
            add("ctx-set:%d" % ctx_set)
            if c1_idx >= C1FLAG_NUMBER:
                add("c1-idx:ge-8")
            if c2_idx >= C2FLAG_NUMBER:
                add("c2-idx:ge-1")
            one_i = base_one + 4 * ctx_set + c1
            abs_i = base_abs + ctx_set + c2
            if scanpos == last_scanpos:
                add("pos:last")
                level = _coded_level(t, scanpos, level_double, max_abs_level, base_sig, one_i, abs_i, rice, c1_idx, c2_idx, temp, True)
            else:
                add("pos:not-last")
                pos_y, pos_x = blkpos >> log2, blkpos & (width - 1)
                sig_i = base_sig + _sig_ctx_inc(pattern, scan_mode, pos_x, pos_y, log2, type_)
                level = _coded_level(t, scanpos, level_double, max_abs_level, sig_i, one_i, abs_i, rice, c1_idx, c2_idx, temp, False)
                if signhide:
                    t.sig_coeff_inc[blkpos] = _bits(t, sig_i, 1) - _bits(t, sig_i, 0)
            if forget in ("cost_coeff", "cost_sig") and scanpos == last_scanpos:
                getattr(t, forget)[scanpos] = UNWRITTEN
            if level < max_abs_level:
                add("level:below-max" if level else "level:zero-from-nonzero-max")
            if signhide:
                t.quant_delta[blkpos] = (level_double - level * (1 << q_bits)) >> (q_bits - 8)
                if level > 0:
                    now = _ic_rate(t, level, one_i, abs_i, rice, c1_idx, c2_idx, False)
                    t.inc[blkpos] = _ic_rate(t, level + 1, one_i, abs_i, rice, c1_idx, c2_idx, False) - now
                    t.dec[blkpos] = _ic_rate(t, level - 1, one_i, abs_i, rice, c1_idx, c2_idx, level == 1) - now
                else:
                    t.inc[blkpos] = _bits(t, one_i, 0)
            dest[blkpos] = UNWRITTEN if forget == "dest" and scanpos == last_scanpos else _i16(level)
            base_cost += t.cost_coeff[scanpos]

            base_level = (2 + (1 if c2_idx < C2FLAG_NUMBER else 0)) if c1_idx < C1FLAG_NUMBER else 1
            if level >= base_level:
                grows = level >= 3 * (1 << rice) if mutant == "rice-threshold-ge" else level > 3 * (1 << rice)
                if grows:
                    add("rice:capped-at-4" if rice == 4 else "rice:raised")
                    rice = min(rice + 1, 5 if mutant == "rice-cap-5" else 4)
            if level >= 1:
                c1_idx += 1
            if level > 1:
                c1 = 0
                c2 += 1 if c2 < 2 else 0
                c2_idx += 1
            elif 0 < c1 < 3 and level:
                c1 += 1
            if scanpos % 16 == 0 and scanpos > 0:               # context set update, rdo.c:732-743
                c2 = rice = c1_idx = c2_idx = 0
                ctx_set = 0 if scanpos == 16 or type_ != 0 else 2
                if c1 == 0 and mutant != "ctx-set-no-bump":
                    ctx_set += 1
                c1 = 1
            sig_cost += t.cost_sig[scanpos]
            if scanpos_in_cg == 0:
                sig_cost_0 = t.cost_sig[scanpos]
            if dest[blkpos]:
                sig_coeffgroup_flag[cg_blkpos] = 1
                coded_level_and_dist += t.cost_coeff[scanpos] - t.cost_sig[scanpos]
                uncoded_dist += t.cost_coeff0[scanpos]
                if scanpos_in_cg != 0:
                    nnz_before_pos0 += 1

        if cg_scanpos:                                          # rdo.c:759-812
            cg_ctx = SIG_CG + type_ + (right | lower)           # kvz_context_get_sig_coeff_group, context.c:303-315
            if sig_coeffgroup_flag[cg_blkpos] == 0:
                add("cg:found-empty")
                cost_coeffgroup_sig[cg_scanpos] = t.lam * _bits(t, cg_ctx, 0)
                base_cost += cost_coeffgroup_sig[cg_scanpos] - sig_cost
            elif cg_scanpos < cg_last_scanpos:
                if nnz_before_pos0 == 0:
                    add("cg:nnz-before-pos0-is-0")
                    if mutant != "nnz-before-pos0-ignored":
                        base_cost -= sig_cost_0
                        sig_cost -= sig_cost_0
                cost_zero_cg = base_cost
                cost_coeffgroup_sig[cg_scanpos] = t.lam * _bits(t, cg_ctx, 1)
                base_cost += cost_coeffgroup_sig[cg_scanpos]
                cost_zero_cg += t.lam * _bits(t, cg_ctx, 0)
                cost_zero_cg += uncoded_dist
                cost_zero_cg -= coded_level_and_dist
                cost_zero_cg -= sig_cost
                if cost_zero_cg < base_cost and mutant != "no-group-zeroing":
                    add("cg:zeroed")
                    sig_coeffgroup_flag[cg_blkpos] = 0
                    base_cost = cost_zero_cg
                    cost_coeffgroup_sig[cg_scanpos] = t.lam * _bits(t, cg_ctx, 0)
                    for scanpos_in_cg in range(15, -1, -1):
                        scanpos = cg_scanpos * 16 + scanpos_in_cg
                        blkpos = scan[scanpos]
                        if dest[blkpos]:
                            dest[blkpos] = 0
                            t.cost_coeff[scanpos] = t.cost_coeff0[scanpos]
                            t.cost_sig[scanpos] = 0.0
                else:
                    add("cg:kept")
        else:
            sig_coeffgroup_flag[cg_blkpos] = 1

    # ===== the last position, rdo.c:815-864
    best_last_idx_p1 = 0
    if block_type != CU_INTRA and not type_ and mutant != "root-cbf-ignored":
        add("cbf:root")
        best_cost = block_uncoded_cost + t.lam * _bits(t, ROOT_CBF, 0)
        base_cost += t.lam * _bits(t, ROOT_CBF, 1)
    else:
        if type_:
            add("cbf:qt-chroma")
            cbf_i = QT_CBF_CHROMA + tr_depth
        else:
            add("cbf:qt-luma-deeper" if tr_depth else "cbf:qt-luma-depth-0")
            cbf_i = QT_CBF_LUMA + (tr_depth if mutant == "luma-cbf-by-depth" else (0 if tr_depth else 1))
        best_cost = block_uncoded_cost + t.lam * _bits(t, cbf_i, 0)
        base_cost += t.lam * _bits(t, cbf_i, 1)
    found_last = False
    for cg_scanpos in range(cg_last_scanpos, -1, -1):
        cg_blkpos = scan_cg[cg_scanpos]
        base_cost -= cost_coeffgroup_sig[cg_scanpos]
        if sig_coeffgroup_flag[cg_blkpos]:
            for scanpos_in_cg in range(15, -1, -1):
                scanpos = cg_scanpos * 16 + scanpos_in_cg
                if scanpos > last_scanpos:
                    continue
                blkpos = scan[scanpos]
                if dest[blkpos]:
                    pos_y, pos_x = blkpos >> log2, blkpos & (width - 1)
                    if scan_mode == SCAN_VER:
                        add("last:vertical-swap")
                    if scan_mode == SCAN_VER and mutant != "no-vertical-swap":
                        cost_last = _rate_last(t, pos_y, pos_x)
                    else:
                        cost_last = _rate_last(t, pos_x, pos_y)
                    total = base_cost + cost_last - t.cost_sig[scanpos]
                    if total < best_cost and mutant != "no-last-search":
                        best_last_idx_p1 = scanpos + 1
                        best_cost = total
                    if dest[blkpos] > 1 and mutant != "found-last-ignored":
                        add("last:found-last")
                        found_last = True
                        break
                    base_cost -= t.cost_coeff[scanpos]
                    base_cost += t.cost_coeff0[scanpos]
                elif mutant != "cost-sig-of-zero-levels-kept":
                    base_cost -= t.cost_sig[scanpos]
            if found_last:
                break
    if mutant == "no-last-search":
        best_last_idx_p1 = last_scanpos + 1
    last_nonzero = max([s for s in range(last_scanpos + 1) if dest[scan[s]]], default=-1)
    add("last:tu-emptied" if best_last_idx_p1 == 0 else "last:kept" if best_last_idx_p1 == last_nonzero + 1 else "last:moved")

    abs_sum = 0
    for scanpos in range(best_last_idx_p1):
        blkpos = scan[scanpos]
        level = dest[blkpos]
        abs_sum += level
        dest[blkpos] = _i16(-level if coef[blkpos] < 0 else level)
    for scanpos in range(best_last_idx_p1, last_scanpos + 1):   # clean uncoded coefficients
        dest[scan[scanpos]] = 0
    if not signhide:
        add("sh:off")
    elif abs_sum < 2:
        add("sh:abs-sum-below-2")
    else:
        _sign_hiding(t, qp_scaled, scan, best_last_idx_p1, coef, dest)
    return dest


def census_counter():
    return collections.Counter()

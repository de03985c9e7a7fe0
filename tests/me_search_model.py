"""A plain model of the motion search of one PU, written from the reference's search_inter.c (and rdo.c for --mv-rdo), with a census of
the decisions it takes and a set of mutants, each one deliberate error in the model.  It covers what ref_me_search_pu
(oracle/ref_me_harness.c) covers:

    fracmv_within_tile            search_inter.c:87-172      _Search.within
    check_mv_cost                 :195-232                   _Search.check
    get_ep_ex_golomb_bitcost      :235-253                   _Search.golomb
    mv_in_merge                   :260-273                   _Search.in_merge
    select_starting_point         :282-307                   _Search.start
    get_mvd_coding_cost           :310-323                   _Search.mvd_bits
    select_mv_cand                :326-370                   _Search.select_cand
    calc_mvd_cost                 :373-412                   _Search.bits
    early_terminate               :415-460                   _Search.early_terminate
    kvz_tz_pattern_search         :463-577                   _Search.tz_pattern (pattern type 0, the only one tz_search uses)
    tz_search                     :595-671                   _Search.tz
    hexagon_search                :690-778                   _Search.hexagon
    diamond_search                :796-883                   _Search.diamond
    search_mv_full                :886-956                   _Search.full
    search_frac                   :965-1128                  _Search.frac (control flow; the samples and their SATD are the oracle's)
    search_pu_inter_ref           :1236-1273                 _Search.run (the gate on *inter_cost, merged / merge_idx / mv_cand)
    kvz_calc_mvd_cost_cabac       rdo.c:908-1060             _Search.bits_cabac
    kvz_get_mvd_coding_cost_cabac rdo.c:883-903              _Search.mvd_bits_cabac

Arithmetic: Python's // floors where C's / truncates, so every division of the reference is written with cdiv(); C's >> on a negative int
is an arithmetic shift (a floor), which is what Python's >> does, and is written asr() where the operand can be negative.  Costs are
uint32 like the reference's.  The SAD is a sum over the edge-replicated reference (clamped indices, image.c:320-444) in int64.

Census: a counter per decision class, named by a string and incremented where the decision is taken (census_classes() lists them all).
Mutants: search_pu(..., mutant=name) makes the one error MUTANTS[name] describes.  Nothing here runs a kernel.  Errors that cannot change a
result are no mutants, because no case could catch them: pricing a point a second time (the diamond's from_dir not skipped, extra_mv added
although it is a merge candidate, the zero window not counted as tested, distance 1 of the tz pattern with eight points) changes nothing
under the strict comparison of check_mv_cost."""
import collections

import numpy as np

import oracle_lib as O
from patterns import ME_RESULT

MAX_INT = 2147483647
U32 = 0xFFFFFFFF

LARGE_HEXBS = ((0, 0), (1, -2), (2, 0), (1, 2), (-1, 2), (-2, 0), (-1, -2), (1, -2), (2, 0))          # :700-704
SMALL_HEXBS = ((0, 0), (0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))          # :709-713
ET_HEXBS = ((0, -1), (-1, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (0, 0))                               # :417-420
DIAMOND = ((0, -1), (1, 0), (0, 1), (-1, 0), (0, 0))                                                  # :810-813
SQUARE = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))               # :971-975
TZ_RANGE = 96                                                                                         # :598
SIDES = ("left", "right", "top", "bottom")
GROUPS_OF_PATTERNS = ("start", "et1", "et2", "hex6", "hex3", "hexsmall", "dia5", "dia3", "tz4", "tz8", "full", "frac")
ME_GROUP = 64                                              # positions the kernel prices per round of its exhaustive search


def cdiv(a, b):
    """C's a / b: truncation toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def asr(a, n):
    """C's a >> n on a signed int (gcc, clang: arithmetic), i.e. floor(a / 2^n)"""
    return a >> n


def wrap16(v):
    """the value an int16 would hold"""
    return ((v + 32768) & 0xFFFF) - 32768


def win_bytes(maxw):
    """the LDS bytes the kernel has for an exhaustive-search window: WIN_BYTES of search_pu_core from frac_geom<MAXW> (frac_core.h)"""
    ps = pr = maxw + 8
    p_bytes = ps * pr + 16
    cur_bytes = maxw * maxw
    h_elems = (maxw + 4) * (maxw + 10)
    h_off = (p_bytes + cur_bytes + 15) & ~15
    total = h_off + 4 * h_elems * 2 + 32
    return total - (p_bytes + cur_bytes)


def size_class(w, h):
    """kvz_hip_me_params.size_classes: 1 = up to 16x16, 2 = up to 32x32, 4 = larger"""
    return 4 if (w > 32 or h > 32) else 2 if (w > 16 or h > 16) else 1


def window_fits(w, h, rng):
    """begin_window of search_pu_core: the (w + 2R) x (h + 2R) window goes to LDS when stride * rows <= WIN_BYTES"""
    stride, rows = ((w + 2 * rng + 3) & ~3) + 4, h + 2 * rng
    return stride * rows <= win_bytes({1: 16, 2: 32, 4: 64}[size_class(w, h)])


# ---------------------------------------------------------------- census
def census_classes():
    c = []
    c += ["start:extra:%s" % k for k in ("zero", "in-merge", "added")]
    c += ["start:merge:%s" % k for k in ("unusable", "zero", "added")]
    c += ["start:winner:%s" % k for k in ("zero", "extra", "merge0", "merge1", "merge2", "merge3", "merge4")]
    c += ["start:duplicate", "start:none-admissible"]
    c += ["check:refused", "check:sad-not-better", "check:cost-not-better", "check:better"]
    c += ["et:level%d" % k for k in range(3)]
    c += ["et:r1:ends", "et:r1:improved-but-ends", "et:r2:ends", "et:r2:continues", "et:l2:equal-threshold"]
    c += ["et:r1:win%d" % k for k in range(4)]
    c += ["et:r2:after%d:none" % b for b in range(4)]
    c += ["et:r2:after%d:p%d" % (b, k) for b in range(4) for k in range(3)]
    c += ["hex:ring1:none"] + ["hex:ring1:win%d" % k for k in range(1, 7)]
    c += ["hex:from%d" % k for k in range(1, 9)]
    c += ["hex:steps:%s" % k for k in ("zero", "one", "ran-out", "exactly-enough", "not-needed", "unlimited")]
    c += ["hex:small:none"] + ["hex:small:win%d" % k for k in range(1, 9)]
    c += ["dia:first:centre"] + ["dia:first:win%d" % k for k in range(4)]
    c += ["dia:skip:from%d" % k for k in range(4)]
    c += ["dia:loop:none"] + ["dia:loop:win%d" % k for k in range(4)]
    c += ["dia:steps:%s" % k for k in ("zero", "one", "ran-out", "unlimited")]
    c += ["tz:best-dist:%d" % (1 << k) for k in range(7)]
    c += ["tz:run1:break3", "tz:run1:to-end", "tz:run2:absent", "tz:run2:present", "tz:run2:break3", "tz:run2:to-end", "tz:run2:improves"]
    c += ["tz:refine:0", "tz:refine:1", "tz:refine:2+"]
    c += ["tz:outside:%s" % s for s in SIDES]
    c += ["full:extra:window", "full:extra:in-merge"]
    c += ["full:merge%d:%s" % (i, k) for i in range(5) for k in ("window", "unusable", "zero")]
    c += ["full:jump:zero-window"] + ["full:jump:merge%d" % j for j in range(4)]
    c += ["full:unusable-earlier-not-counted", "full:within-false", "full:last-group-short"]
    c += ["full:lds:%d:%s" % (m, k) for m in (16, 32, 64) for k in ("fits", "no-fit")]
    c += ["full:winner:%s" % k for k in ("zero-window", "extra-window", "merge-window")]
    c += ["tie:%s:%s" % (g, k) for g in GROUPS_OF_PATTERNS for k in ("first-wins", "equals-incumbent")]
    c += ["cost:merged:idx%d" % i for i in range(5)]
    c += ["cost:merge:usable-not-same-ref", "cost:merge:duplicate", "cost:merge:wrapped-equal-outside-int16"]
    c += ["cost:amvp:%s" % k for k in ("first", "second", "tie", "same-cands")]
    c += ["cost:golomb:2^%d%s" % (k, s) for k in range(2, 16) for s in ("-1", "+0", "+1")]
    c += ["cost:golomb:fallback-x", "cost:golomb:fallback-y"]
    c += ["cost:lambda:0", "cost:lambda:2^20"]
    c += ["within:c0"] + ["within:c%d:refused:%s" % (k, s) for k in range(1, 5) for s in SIDES] + ["within:c%d:pass" % k for k in range(1, 5)]
    c += ["within:margin:%s" % k for k in ("int", "chroma-frac", "luma-frac")]
    c += ["within:c4:margin-alone-refuses:%s" % k for k in ("chroma-frac", "luma-frac")]
    c += ["within:wpp:%s" % k for k in ("pass", "refused-down", "refused-sum", "neg-numerator", "delay-deblock", "delay-sao", "delay-none")]
    c += ["frac:level%d" % k for k in range(5)]
    c += ["frac:gate:%s" % k for k in ("open", "closed", "equal")]
    c += ["frac:skipped-no-start"]
    c += ["frac:hpel:win%d" % k for k in range(9)] + ["frac:qpel:win%d" % k for k in range(9)]
    c += ["frac:refused-would-have-won"]
    c += ["shape:%s" % k for k in ("8x8", "16x16", "32x32", "generic-small", "generic-medium", "generic-big", "w4", "w12", "segs-not-pow2",
                                   "64x64", "big-amp")]
    c += ["border:%s" % s for s in SIDES] + ["border:wholly-outside"]
    c += ["rdo:merged", "rdo:not-merged", "rdo:refs1", "rdo:refs2", "rdo:refs>2", "rdo:ref-idx0", "rdo:ref-idx>0"]
    c += ["rdo:ctx%d:%s" % (k, s) for k in range(7) for s in ("mps", "lps")]
    c += ["rdo:select:cand0", "rdo:select:cand1", "rdo:select:same-cands"]
    c += ["result:merged", "result:not-merged"]
    return c


_CLASSES = frozenset(census_classes())

# classes nothing can reach, each with the reason
UNREACHABLE = {
    "tie:start:equals-incumbent": "select_starting_point begins from best_cost = UINT32_MAX (:715, :815, :607) and no cost reaches it: lambda_cost <= 2^20 "
                                  "and fewer than 2^7 bits",
    "full:lds:64:no-fit": "the entry allows search_range <= 64 and PUs up to 64x64: the largest window, 196 x 192 bytes, is below WIN_BYTES of frac_geom<64>",
}

GROUPS = ("start", "et", "hex", "dia", "tz", "full", "decide", "cost", "within", "frac", "border", "rdo")
_MUTANT_TABLE = [
    # start points
    ("start-merge-plain-shift", "start", "merge start points by mv >> 2 instead of (mv + 2) >> 2 (:300-301)"),
    ("start-extra-rounded", "start", "extra_mv by (mv + 2) >> 2 instead of mv >> 2 (:288-289)"),
    ("start-unusable-checked", "start", "a merge candidate with dir == 3 is checked as a start point (:298)"),
    # early termination
    ("et-threshold-gt", "et", "best_cost > threshold instead of >= (:452)"),
    ("et-first-index", "et", "the second round starts at (best_index + 2) % 4 (:456)"),
    ("et-l2-as-l1", "et", "the sensitive level's threshold is best_cost, not 0.95 best_cost (:432)"),
    ("et-one-round", "et", "one round instead of two (:427)"),
    # hexagon
    ("hex-wrap1", "hex", "best_index 1 starts at 0 instead of 6 (:748-749)"),
    ("hex-wrap8", "hex", "best_index 8 starts at 2 instead of 1 (:750-751)"),
    ("hex-steps-plus-one", "hex", "one more step than max_steps allows (:742)"),
    ("hex-small-7", "hex", "the last of the eight small points is left out (:775)"),
    ("hex-centre-not-moved", "hex", "the centre does not move to the best match before the three new points (:757-758)"),
    # diamond
    ("dia-from-dir-not-flipped", "dia", "from_dir = best_index instead of best_index ^ 3 (:879): the way ahead is skipped"),
    ("dia-maxsteps0-no-round", "dia", "max_steps == 0 runs no round of the loop (:856-881 is a do-while)"),
    ("dia-steps-plus-one", "dia", "one more round than max_steps allows (:881)"),
    # tz
    ("tz-rounds-2", "tz", "the grid search breaks after two rounds without improvement (:629, :641)"),
    ("tz-second-run-from-start", "tz", "the second grid run starts from the start vector, not from (0, 0) (:634-635)"),
    ("tz-second-run-96", "tz", "the second grid run goes to distance 96 instead of 48 (:637)"),
    ("tz-no-refinement", "tz", "no star refinement (:663-670)"),
    ("tz-refine-once", "tz", "the star refinement runs once at the most (:663)"),
    ("tz-to-64", "tz", "the first grid run and the refinement stop before distance 64 (:624, :667)"),
    # exhaustive search
    ("full-jump-plus-one", "full", "the jump past an earlier window lands one position too far (:946)"),
    ("full-unusable-window-counted", "full", "the window of an unusable earlier candidate counts as tested (:938)"),
    ("full-rounded-shift", "full", "window centres by (mv + 2) >> 2 instead of mv >> 2 (:916-917)"),
    ("full-extra-in-merge-searched", "full", "the window around extra_mv is searched from (mv + 2) >> 2 of it (:898-899)"),
    # the rule of every group
    ("last-wins", "decide", "of two candidates that tie for a group's minimum the later one wins"),
    ("le-incumbent", "decide", "a candidate that equals the incumbent replaces it (:211, :223, :1095)"),
    # cost model
    ("merge-no-range-check", "cost", "merge matching compares 16-bit values: a vector outside int16 matches at its wrapped value (:393-394)"),
    ("golomb-fast-past-2^16", "cost", "2 floor(log2(symbol + 2)) also at 2^16 and above (:241-244 add up to less there)"),
    ("merge-ignores-same-ref", "cost", "a usable merge candidate matches whatever its reference (:395-397)"),
    ("merge-last-match", "cost", "of two equal merge candidates the later index is coded (:400)"),
    ("amvp-tie-second", "cost", "cand2_cost <= cand1_cost picks the second candidate (:369)"),
    ("merge-idx-plus-one", "cost", "a merged vector costs merge_idx + 1 bits (:398)"),
    ("lambda-20-bits", "cost", "the multiplier keeps 20 bits of lambda_cost: 2^20 becomes 0 (:411)"),
    ("golomb-at-power-off", "cost", "symbol + 2 > 2^k instead of >= in the four range tests (:241-244)"),
    # within
    ("wpp-floor-division", "within", "the LCU index of the WPP rule by floor instead of truncation (:127-128)"),
    ("c3-with-c4-margins", "within", "FRAME_AND_TILE gets the margins of FRAME_AND_TILE_MARGIN (:148)"),
    ("c4-without-margins", "within", "FRAME_AND_TILE_MARGIN without its margins (:148-154)"),
    ("wpp-margin-no-frac", "within", "the WPP rule without the 4 / 2 pixel margin of fractional vectors (:98-107)"),
    ("wpp-delay-ignored", "within", "the WPP rule without SAO_DELAY_PX / DEBLOCK_DELAY_PX (:109-116)"),
    ("wpp-sum-rule-dropped", "within", "only mv_lcu.y > down is tested (:135-139)"),
    ("wpp-down-rule-dropped", "within", "only the sum rule is tested (:131-133)"),
    ("within-right-gt", "within", "from_right > margin instead of >= (:170)"),
    ("within-top-gt", "within", "abs_mv.y > margin instead of >= (:169)"),
    ("within-tile-origin-ignored", "within", "the PU's origin taken in the picture, not in the tile (:157-160)"),
    # fractional stage
    ("gate-le", "frac", "best_cost <= *inter_cost opens the fractional stage (:1239)"),
    ("frac-le", "frac", "costs[j] <= best_cost in the fractional stage (:1095)"),
    ("frac-within-ignored", "frac", "fractional candidates are not tested with fracmv_within_tile (:1064-1068)"),
    ("frac-qpel-around-integer", "frac", "the quarter-pel steps search around the integer vector (:1107-1108)"),
    ("frac-no-bits", "frac", "fractional candidates are priced without their bits (:1078-1092)"),
    ("frac-level-as-4", "frac", "every fme_level > 0 runs all four steps (:1046)"),
    # picture borders
    ("border-clamp-short", "border", "reference columns and rows are clamped one short of the last (image.c:320-444)"),
    ("border-no-clamp-top", "border", "rows above the picture read row 1, not row 0"),
    # --mv-rdo
    ("rdo-refs-before-ignored", "rdo", "ref_idx is never coded (rdo.c:1004)"),
    ("rdo-merge-idx-short", "rdo", "merge_idx is coded with one bin (rdo.c:978-992)"),
    ("rdo-select-first", "rdo", "the result's mv_cand is always 0 with --mv-rdo (:343-344)"),
    ("rdo-mvp-bin-dropped", "rdo", "the mvp index bin is not counted (rdo.c:1040)"),
    ("rdo-lps-no-renorm", "rdo", "an LPS counts one bit (cabac.c:104-113)"),
]
MUTANTS = {m[0]: m[2] for m in _MUTANT_TABLE}
MUTANT_GROUP = {m[0]: m[1] for m in _MUTANT_TABLE}


# ---------------------------------------------------------------- CABAC tables (ITU-T H.265 Tables 9-46, 9-47), read from the oracle
_CABAC = {}


def _cabac_tables():
    if not _CABAC:
        L = O.lib()
        L.orc_cabac_table.restype = int
        _CABAC["lps"] = [[L.orc_cabac_table(0, 4 * s + q) for q in range(4)] for s in range(64)]
        _CABAC["mps_next"] = [L.orc_cabac_table(1, uc) for uc in range(128)]
        _CABAC["lps_next"] = [L.orc_cabac_table(2, uc) for uc in range(128)]
        _CABAC["renorm"] = [L.orc_cabac_table(3, i) for i in range(32)]
    return _CABAC


class _Cabac:
    """the bits kvz_cabac_encode_bin (cabac.c:90-122) produces in counting mode: the renormalisation shifts"""

    def __init__(self, snapshot, s):
        self.range, self.ctx, self.s, self.t = int(snapshot["range"]), [int(v) for v in snapshot["ctx"]], s, _cabac_tables()

    def bin(self, ctx, b):
        uc = self.ctx[ctx]
        lps = self.t["lps"][uc >> 1][(self.range >> 6) & 3]
        self.range -= lps
        if (1 if b else 0) != (uc & 1):
            self.s.hit("rdo:ctx%d:lps" % ctx)
            n = 1 if self.s.mutant == "rdo-lps-no-renorm" else self.t["renorm"][lps >> 3]
            self.range = lps << self.t["renorm"][lps >> 3]
            self.ctx[ctx] = self.t["lps_next"][uc]
            return n
        self.s.hit("rdo:ctx%d:mps" % ctx)
        self.ctx[ctx] = self.t["mps_next"][uc]
        if self.range >= 256:
            return 0
        self.range <<= 1
        return 1

    @staticmethod
    def ex_golomb(symbol, count):
        """kvz_cabac_write_ep_ex_golomb (cabac.c:535-570): bypass bins"""
        n = 0
        while symbol >= (1 << count):
            n += 1
            symbol -= 1 << count
            count += 1
        return n + 1 + count

    def mvd(self, hor, ver):
        """kvz_encode_mvd (encode_coding_tree.c:1156-1202)"""
        ah, av = abs(hor), abs(ver)
        bits = self.bin(4, hor != 0)
        bits += self.bin(4, ver != 0)
        if hor:
            bits += self.bin(5, ah > 1)
        if ver:
            bits += self.bin(5, av > 1)
        if hor:
            bits += (self.ex_golomb(ah - 2, 1) if ah > 1 else 0) + 1
        if ver:
            bits += (self.ex_golomb(av - 2, 1) if av > 1 else 0) + 1
        return bits


RUNAWAY_CHECKS = 150000          # more candidates than any search of the reference prices: 7 windows of 129 x 129 are 116487


class Runaway(Exception):
    """a mutant's search does not end"""


# ---------------------------------------------------------------- the search of one PU
class _Search:
    def __init__(self, pic, ref, pu, prm, cabac, cost_to_beat, mutant, census, trace):
        assert mutant is None or mutant in MUTANTS, mutant
        self.pic, self.ref, self.mutant, self.census, self.trace = pic, ref, mutant, census, trace
        self.H, self.W = ref.shape
        self.x, self.y, self.w, self.h = int(pu["x"]), int(pu["y"]), int(pu["width"]), int(pu["height"])
        self.cand = [[int(v) for v in c] for c in pu["mv_cand"]]
        self.extra = [int(v) for v in pu["extra_mv"]]
        self.merge = [(int(m["mv"][0]), int(m["mv"][1]), bool(m["usable"]), bool(m["same_ref"])) for m in pu["merge"][:int(pu["num_merge_cand"])]]
        g = lambda k: int(prm[k])
        self.lam, self.et, self.max_steps, self.fme = g("lambda_cost"), g("early_termination"), g("max_steps"), g("fme_level")
        self.wpp, self.delay, self.down, self.right = g("wpp_owf"), g("ref_delay_px"), g("max_ref_lcu_down"), g("max_ref_lcu_right")
        self.alg, self.range, self.constraint = g("algorithm"), g("search_range"), g("mv_constraint")
        self.tile = (g("tile_x"), g("tile_y"), g("tile_w"), g("tile_h"))
        if self.tile[2] == 0 and self.tile[3] == 0:                    # the picture is one tile
            self.tile = (0, 0, self.W, self.H)
        self.rdo, self.ref_idx, self.refs_before = g("mv_rdo"), g("ref_idx"), g("refs_before")
        self.snapshot = cabac[int(pu["reserved"])] if self.rdo else None
        self.cost_to_beat = MAX_INT if cost_to_beat is None else int(cost_to_beat)
        self.cur = np.ascontiguousarray(pic[self.y:self.y + self.h, self.x:self.x + self.w]).astype(np.int64)
        self.best_mv, self.best_cost, self.best_bits = (0, 0), U32, 0     # inter_search_info_t, zero-initialised by the caller
        self.mute = 0
        self.checks = 0
        self.group = None
        self.sad_cache = {}

    # ---- census
    def hit(self, name, n=1):
        if self.mute or self.census is None:
            return
        assert name in _CLASSES, name
        self.census[name] += n

    def begin_group(self, kind):
        self.group, self.g_inc, self.g_costs = kind, self.best_cost, []

    def end_group(self):
        """the rule of every group, counted: the first candidate that reaches the group's minimum wins, if that minimum is below the incumbent"""
        c = self.g_costs
        if c:
            m = min(c)
            if m < self.g_inc and c.count(m) >= 2:
                self.hit("tie:%s:first-wins" % self.group)
            if m == self.g_inc:
                self.hit("tie:%s:equals-incumbent" % self.group)
        self.group = None

    def accepts(self, cost):
        """strictly below the best so far (:211, :223, :1095)"""
        if cost < self.best_cost:
            return True
        if cost == self.best_cost:
            if self.mutant == "last-wins":
                return self.best_cost < self.g_inc               # the best so far is an earlier candidate of this group
            if self.mutant == "le-incumbent":
                return self.best_cost == self.g_inc              # the best so far is the incumbent
        return False

    # ---- fracmv_within_tile (:87-172); x, y in quarter-pel
    def within(self, x, y):
        if not self.wpp and self.constraint == 0:
            self.hit("within:c0")
            return True
        frac_luma, frac_chroma = x % 4 != 0 or y % 4 != 0, x % 8 != 0 or y % 8 != 0       # C's % differs in sign only: != 0 is the same
        ox, oy = self.x - self.tile[0], self.y - self.tile[1]                              # info->origin is relative to the tile
        if self.mutant == "within-tile-origin-ignored":
            ox, oy = self.x, self.y
        if self.wpp:                                                                       # cfg.owf && cfg.wpp (:94-140)
            margin = 4 if frac_luma else 2 if frac_chroma else 0
            if self.mutant == "wpp-margin-no-frac":
                margin = 0
            if self.mutant != "wpp-delay-ignored":
                margin += self.delay                                                       # SAO_DELAY_PX = 10 or DEBLOCK_DELAY_PX = 8 (:109-116)
            self.hit("within:wpp:delay-%s" % {8: "deblock", 10: "sao"}.get(self.delay, "none"))
            div = (lambda a, b: a // b) if self.mutant == "wpp-floor-division" else cdiv
            num_x, num_y = (ox + self.w + margin) * 4 + x, (oy + self.h + margin) * 4 + y
            if num_x < 0 or num_y < 0:
                self.hit("within:wpp:neg-numerator")
            mv_lcu_x = div(num_x, 64 << 2) - cdiv(ox, 64)
            mv_lcu_y = div(num_y, 64 << 2) - cdiv(oy, 64)
            if mv_lcu_y > self.down and self.mutant != "wpp-down-rule-dropped":
                self.hit("within:wpp:refused-down")
                return False
            if mv_lcu_x + mv_lcu_y > self.down + self.right and self.mutant != "wpp-sum-rule-dropped":
                self.hit("within:wpp:refused-sum")
                return False
            self.hit("within:wpp:pass")
        if self.constraint == 0:                                                           # KVZ_MV_CONSTRAIN_NONE (:142-144)
            return True
        margin = 0
        with_margins = self.constraint == 4
        if self.mutant == "c3-with-c4-margins" and self.constraint == 3:
            with_margins = True
        if self.mutant == "c4-without-margins":
            with_margins = False
        if with_margins:                                                                   # KVZ_MV_CONSTRAIN_FRAME_AND_TILE_MARGIN (:148-154)
            margin = 4 << 2 if frac_luma else 2 << 2 if frac_chroma else 0
            self.hit("within:margin:%s" % ("luma-frac" if frac_luma else "chroma-frac" if frac_chroma else "int"))
        ax, ay = ox * 4 + x, oy * 4 + y
        from_right = (self.tile[2] << 2) - (ax + (self.w << 2))
        from_bottom = (self.tile[3] << 2) - (ay + (self.h << 2))
        ok = [ax >= margin, from_right >= margin, ay >= margin, from_bottom >= margin]
        if self.mutant == "within-right-gt":
            ok[1] = from_right > margin
        if self.mutant == "within-top-gt":
            ok[2] = ay > margin
        if all(ok):
            self.hit("within:c%d:pass" % self.constraint)
            return True
        for k in range(4):
            if not ok[k]:
                self.hit("within:c%d:refused:%s" % (self.constraint, SIDES[k]))
        if margin and ax >= 0 and ay >= 0 and from_right >= 0 and from_bottom >= 0:
            self.hit("within:c4:margin-alone-refuses:%s" % ("luma-frac" if frac_luma else "chroma-frac"))
        return False

    # ---- kvz_image_calc_sad (image.c:455-486): a SAD against the edge-replicated reference; x, y integer-pel
    def clamped(self, x0, y0, w, h):
        hi_x, hi_y = (self.W - 2, self.H - 2) if self.mutant == "border-clamp-short" else (self.W - 1, self.H - 1)
        rows, cols = np.clip(np.arange(y0, y0 + h), 0, hi_y), np.clip(np.arange(x0, x0 + w), 0, hi_x)
        if self.mutant == "border-no-clamp-top":
            rows = np.where(np.arange(y0, y0 + h) < 0, 1, rows)
        return self.ref[np.ix_(rows, cols)]

    def note_border(self, bx, by):
        out = (bx < 0, bx + self.w > self.W, by < 0, by + self.h > self.H)
        if not any(out):
            return
        if bx + self.w <= 0 or bx >= self.W or by + self.h <= 0 or by >= self.H:
            self.hit("border:wholly-outside")
        for k in range(4):
            if out[k]:
                self.hit("border:%s" % SIDES[k])
                if self.group in ("tz4", "tz8"):
                    self.hit("tz:outside:%s" % SIDES[k])

    def sad(self, x, y):
        key = (x, y)
        if key not in self.sad_cache:
            blk = self.clamped(self.x + x, self.y + y, self.w, self.h).astype(np.int64)
            self.sad_cache[key] = int(np.abs(blk - self.cur).sum())
        return self.sad_cache[key]

    # ---- get_ep_ex_golomb_bitcost (:235-253)
    def golomb(self, symbol, axis):
        symbol += 2
        if symbol >= 1 << 16:
            self.hit("cost:golomb:fallback-%s" % axis)
            if self.mutant == "golomb-fast-past-2^16":
                return 2 * (symbol.bit_length() - 1)
        else:
            k = symbol.bit_length() - 1                        # 2^k <= symbol < 2^(k+1)
            if symbol == 1 << k and k >= 2:
                self.hit("cost:golomb:2^%d+0" % k)
            if symbol == (1 << k) + 1 and k >= 2:
                self.hit("cost:golomb:2^%d+1" % k)
            if symbol == (1 << (k + 1)) - 1 and 2 <= k + 1 <= 15:
                self.hit("cost:golomb:2^%d-1" % (k + 1))
        ge = (lambda a, b: a > b) if self.mutant == "golomb-at-power-off" else (lambda a, b: a >= b)
        bins = 0
        if ge(symbol, 1 << 8):
            bins += 16
            symbol >>= 8
        if ge(symbol, 1 << 4):
            bins += 8
            symbol >>= 4
        if ge(symbol, 1 << 2):
            bins += 4
            symbol >>= 2
        if ge(symbol, 1 << 1):
            bins += 2
        return bins

    def mvd_bits(self, dx, dy):
        """get_mvd_coding_cost (:310-323): both terms are whole bits, the fixed-point rounding is exact"""
        return self.golomb(abs(dx), "x") + self.golomb(abs(dy), "y")

    def mvd_bits_cabac(self, dx, dy):
        """kvz_get_mvd_coding_cost_cabac (rdo.c:883-903) on a fresh copy of the state"""
        return _Cabac(self.snapshot, self).mvd(dx, dy)

    # ---- select_mv_cand (:326-370)
    def select_cand(self, x, y, want_cost):
        same = self.cand[0] == self.cand[1]
        if same and not want_cost:
            return 0, None
        f = self.mvd_bits_cabac if self.rdo else self.mvd_bits
        c1 = f(x - self.cand[0][0], y - self.cand[0][1])
        c2 = c1 if same else f(x - self.cand[1][0], y - self.cand[1][1])
        if not self.rdo:
            self.hit("cost:amvp:%s" % ("same-cands" if same else "first" if c1 < c2 else "second" if c2 < c1 else "tie"))
        second = c2 <= c1 if (self.mutant == "amvp-tie-second" and not same) else c2 < c1
        return (1 if second else 0), min(c1, c2)

    # ---- the merge match of calc_mvd_cost (:390-402); x, y quarter-pel
    def merge_match(self, x, y):
        found = -1
        if self.mutant == "merge-no-range-check":
            x, y = wrap16(x), wrap16(y)
        for i, (mx, my, usable, same_ref) in enumerate(self.merge):
            if not usable:                                       # dir == 3
                continue
            if mx == x and my == y:
                if not same_ref and self.mutant != "merge-ignores-same-ref":
                    self.hit("cost:merge:usable-not-same-ref")
                    continue
                if found >= 0:
                    self.hit("cost:merge:duplicate")
                    if self.mutant != "merge-last-match":
                        continue
                found = i
        if found < 0 and (x != wrap16(x) or y != wrap16(y)) and any(u and s and mx == wrap16(x) and my == wrap16(y) for mx, my, u, s in self.merge):
            self.hit("cost:merge:wrapped-equal-outside-int16")
        return found

    # ---- calc_mvd_cost (:373-412) / kvz_calc_mvd_cost_cabac (rdo.c:908-1060); x, y in units of 1 << mv_shift quarter-pels
    def bits(self, x, y, mv_shift):
        x, y = x * (1 << mv_shift), y * (1 << mv_shift)
        if self.rdo:
            return self.bits_cabac(x, y)
        m = self.merge_match(x, y)
        if m >= 0:
            self.hit("cost:merged:idx%d" % m)
            return m + (1 if self.mutant == "merge-idx-plus-one" else 0)
        return self.select_cand(x, y, True)[1]

    def bits_cabac(self, x, y):
        m = self.merge_match(x, y)
        cur_cand, mvd = 0, (0, 0)
        if m < 0:                                                # rdo.c:952-972
            d1 = (x - self.cand[0][0], y - self.cand[0][1])
            d2 = (x - self.cand[1][0], y - self.cand[1][1])
            c1, c2 = self.mvd_bits_cabac(*d1), self.mvd_bits_cabac(*d2)
            cur_cand, mvd = (1, d2) if c2 < c1 else (0, d1)
        cab = _Cabac(self.snapshot, self)
        bits = cab.bin(0, m >= 0)                                # rdo.c:976
        if m >= 0:
            self.hit("rdo:merged")
            for ui in range(1 if self.mutant == "rdo-merge-idx-short" else 4):     # MRG_MAX_NUM_CANDS - 1 (rdo.c:978-992)
                symbol = ui != m
                bits += cab.bin(1, symbol) if ui == 0 else 1
                if not symbol:
                    break
        else:
            self.hit("rdo:not-merged")
            self.hit("rdo:refs%s" % ("1" if self.refs_before == 1 else "2" if self.refs_before == 2 else ">2"))
            if self.refs_before > 1 and self.mutant != "rdo-refs-before-ignored":     # rdo.c:1004-1030
                ref_frame = self.ref_idx
                self.hit("rdo:ref-idx%s" % ("0" if ref_frame == 0 else ">0"))
                bits += cab.bin(2, ref_frame != 0)
                if ref_frame > 0:
                    ref_frame -= 1
                    for i in range(self.refs_before - 2):
                        symbol = 0 if i == ref_frame else 1
                        bits += cab.bin(3, symbol) if i == 0 else 1
                        if not symbol:
                            break
            bits += cab.mvd(*mvd)                                # rdo.c:1033-1037
            if self.mutant != "rdo-mvp-bin-dropped":
                bits += cab.bin(6, cur_cand)                     # kvz_cabac_write_unary_max_symbol(.., cur_mv_cand, 1, 1): one bin
        return bits

    def price(self, bits):
        """temp_bitcost * (int32_t)(lambda_sqrt + 0.5) in uint32 (:411)"""
        lam = self.lam & 0xFFFFF if self.mutant == "lambda-20-bits" else self.lam
        return (bits * lam) & U32

    # ---- check_mv_cost (:195-232); x, y integer-pel
    def check(self, x, y, sad=None):
        self.checks += 1
        if self.mutant and self.checks > (RUNAWAY_CHECKS if self.alg == 3 else RUNAWAY_CHECKS // 30):     # accepting equal costs can walk in circles for ever
            raise Runaway(self.mutant)
        if not self.within(x * 4, y * 4):
            self.hit("check:refused")
            if self.group == "full":
                self.hit("full:within-false")
            return False
        self.note_border(self.x + x, self.y + y)
        if sad is None:
            sad = self.sad(x, y)
        if self.group is not None and sad <= self.g_inc:
            self.mute += 1
            self.g_costs.append((sad + self.price(self.bits(x, y, 2))) & U32)
            self.mute -= 1
        if not self.accepts(sad):
            self.hit("check:sad-not-better")
            return False
        bits = self.bits(x, y, 2)
        cost = (sad + self.price(bits)) & U32
        if not self.accepts(cost):
            self.hit("check:cost-not-better")
            return False
        self.hit("check:better")
        if self.trace is not None:
            self.trace.append("%s: (%d, %d) cost %d bits %d" % (self.group, x, y, cost, bits))
        self.best_mv, self.best_cost, self.best_bits = (x * 4, y * 4), cost, bits
        return True

    # ---- mv_in_merge (:260-273); integer-pel
    def in_merge(self, x, y):
        for mx, my, usable, _ in self.merge:
            if usable and asr(mx + 2, 2) == x and asr(my + 2, 2) == y:
                return True
        return False

    # ---- select_starting_point (:282-307)
    def start(self):
        self.begin_group("start")
        points = [("zero", 0, 0)]
        ex, ey = asr(self.extra[0], 2), asr(self.extra[1], 2)
        if self.mutant == "start-extra-rounded":
            ex, ey = asr(self.extra[0] + 2, 2), asr(self.extra[1] + 2, 2)
        if ex == 0 and ey == 0:
            self.hit("start:extra:zero")
        elif self.in_merge(ex, ey):
            self.hit("start:extra:in-merge")
        else:
            self.hit("start:extra:added")
            points.append(("extra", ex, ey))
        for i, (mx, my, usable, _) in enumerate(self.merge):
            if not usable and self.mutant != "start-unusable-checked":
                self.hit("start:merge:unusable")
                continue
            x, y = (asr(mx, 2), asr(my, 2)) if self.mutant == "start-merge-plain-shift" else (asr(mx + 2, 2), asr(my + 2, 2))
            if x == 0 and y == 0:
                self.hit("start:merge:zero")
                continue
            self.hit("start:merge:added")
            points.append(("merge%d" % i, x, y))
        if len({(x, y) for _, x, y in points}) < len(points):
            self.hit("start:duplicate")
        winner = None
        for name, x, y in points:
            if self.check(x, y):
                winner = name
        self.hit("start:winner:%s" % winner if winner else "start:none-admissible")
        self.end_group()

    # ---- early_terminate (:415-460)
    def early_terminate(self):
        mvx, mvy = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
        first, last = 0, 3
        for k in range(1 if self.mutant == "et-one-round" else 2):
            sensitive = self.et == 2 and self.mutant != "et-l2-as-l1"           # KVZ_ME_EARLY_TERMINATION_SENSITIVE
            threshold = self.best_cost * 0.95 if sensitive else float(self.best_cost)      # a double
            before = self.best_cost
            self.begin_group("et%d" % (k + 1))
            best_index = 6
            for i in range(first, last + 1):
                if self.check(mvx + ET_HEXBS[i][0], mvy + ET_HEXBS[i][1]):
                    best_index = i
            self.end_group()
            mvx, mvy = mvx + ET_HEXBS[best_index][0], mvy + ET_HEXBS[best_index][1]
            if k == 0:
                if best_index != 6:
                    self.hit("et:r1:win%d" % best_index)
                prev = best_index
            else:
                self.hit("et:r2:after%d:%s" % (prev % 4, "none" if best_index == 6 else "p%d" % (best_index - first)))
            ends = self.best_cost > threshold if self.mutant == "et-threshold-gt" else self.best_cost >= threshold
            if sensitive and self.best_cost == threshold and self.best_cost < before:
                self.hit("et:l2:equal-threshold")
            if ends:
                self.hit("et:r%d:ends" % (k + 1))
                if k == 0 and best_index != 6:
                    self.hit("et:r1:improved-but-ends")
                return True
            first = (best_index + (2 if self.mutant == "et-first-index" else 3)) % 4
            last = first + 2
        self.hit("et:r2:continues")
        return False

    def opening(self):
        """the common opening of the three pattern searches (:715-726, :815-826, :606-618): True when the search is over"""
        self.best_cost = U32
        self.start()
        self.hit("et:level%d" % self.et)
        return bool(self.et) and self.early_terminate()

    # ---- hexagon_search (:690-778)
    def hexagon(self):
        if self.opening():
            return
        mvx, mvy = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
        best_index, steps = 0, self.max_steps
        if self.mutant == "hex-steps-plus-one" and steps != U32:
            steps += 1
        self.begin_group("hex6")
        for i in range(1, 7):
            if self.check(mvx + LARGE_HEXBS[i][0], mvy + LARGE_HEXBS[i][1]):
                best_index = i
        self.end_group()
        self.hit("hex:ring1:win%d" % best_index if best_index else "hex:ring1:none")
        needed = best_index != 0
        while best_index != 0 and steps != 0:
            if steps > 0:
                steps -= 1
            self.hit("hex:from%d" % best_index)
            if best_index == 1:
                start = 0 if self.mutant == "hex-wrap1" else 6
            elif best_index == 8:
                start = 2 if self.mutant == "hex-wrap8" else 1
            else:
                start = best_index - 1
            if self.mutant != "hex-centre-not-moved":
                mvx, mvy = mvx + LARGE_HEXBS[best_index][0], mvy + LARGE_HEXBS[best_index][1]
            best_index = 0
            self.begin_group("hex3")
            for i in range(3):
                if self.check(mvx + LARGE_HEXBS[start + i][0], mvy + LARGE_HEXBS[start + i][1]):
                    best_index = start + i
            self.end_group()
        if self.max_steps == U32:
            self.hit("hex:steps:unlimited")
        elif best_index != 0:
            self.hit("hex:steps:%s" % {0: "zero", 1: "one"}.get(self.max_steps, "ran-out"))
        elif needed and steps == 0:
            self.hit("hex:steps:exactly-enough")
        else:
            self.hit("hex:steps:not-needed")
        self.begin_group("hexsmall")
        winner = 0
        for i in range(1, 8 if self.mutant == "hex-small-7" else 9):
            if self.check(mvx + SMALL_HEXBS[i][0], mvy + SMALL_HEXBS[i][1]):
                winner = i
        self.end_group()
        self.hit("hex:small:win%d" % winner if winner else "hex:small:none")

    # ---- diamond_search (:796-883)
    def diamond(self):
        if self.opening():
            return
        mvx, mvy = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
        best_index, steps = 4, self.max_steps
        if self.mutant == "dia-steps-plus-one" and steps != U32:
            steps += 1
        self.begin_group("dia5")
        for i in range(5):
            if self.check(mvx + DIAMOND[i][0], mvy + DIAMOND[i][1]):
                best_index = i
        self.end_group()
        if best_index == 4:
            self.hit("dia:first:centre")
            return
        self.hit("dia:first:win%d" % best_index)
        mvx, mvy = mvx + DIAMOND[best_index][0], mvy + DIAMOND[best_index][1]
        from_dir = 4
        if self.mutant == "dia-maxsteps0-no-round" and steps == 0:
            return
        while True:                                              # do { } while (better_found && steps != 0)
            better = False
            if steps > 0:
                steps -= 1
            self.begin_group("dia3")
            for i in range(4):
                if i == from_dir:
                    self.hit("dia:skip:from%d" % i)
                    continue
                if self.check(mvx + DIAMOND[i][0], mvy + DIAMOND[i][1]):
                    best_index, better = i, True
            self.end_group()
            self.hit("dia:loop:win%d" % best_index if better else "dia:loop:none")
            if better:
                mvx, mvy = mvx + DIAMOND[best_index][0], mvy + DIAMOND[best_index][1]
                from_dir = best_index if self.mutant == "dia-from-dir-not-flipped" else best_index ^ 3
            if not (better and steps != 0):
                break
        if self.max_steps == U32:
            self.hit("dia:steps:unlimited")
        elif better:
            self.hit("dia:steps:%s" % {0: "zero", 1: "one"}.get(self.max_steps, "ran-out"))

    # ---- kvz_tz_pattern_search (:463-577), pattern_type 0: the 8-point diamond, 4 points at distance 1
    def tz_pattern(self, dist, sx, sy, best_dist):
        hd = cdiv(dist, 2)
        pattern = ((0, dist), (dist, 0), (0, -dist), (-dist, 0), (hd, hd), (hd, -hd), (-hd, -hd), (-hd, hd))
        n = 4 if dist == 1 else 8
        self.begin_group("tz%d" % n)
        improved = False
        for i in range(n):
            if self.check(sx + pattern[i][0], sy + pattern[i][1]):
                improved = True
        self.end_group()
        if improved:
            self.hit("tz:best-dist:%d" % dist)
            return dist
        return best_dist

    # ---- tz_search (:595-671): range 96, diamond patterns, no raster scan, star refinement
    def tz(self):
        best_dist = 0
        if self.opening():
            return
        sx, sy = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
        limit = 3 if self.mutant != "tz-rounds-2" else 2
        top = 63 if self.mutant == "tz-to-64" else TZ_RANGE
        rounds, dist, broke = 0, 1, False
        while dist <= top:
            best_dist = self.tz_pattern(dist, sx, sy, best_dist)
            if best_dist != dist:
                rounds += 1
            if rounds >= limit:
                broke = True
                break
            dist *= 2
        self.hit("tz:run1:break3" if broke else "tz:run1:to-end")
        if sx != 0 or sy != 0:
            self.hit("tz:run2:present")
            if self.mutant != "tz-second-run-from-start":
                sx, sy = 0, 0
            rounds, dist, broke = 0, 1, False
            while dist <= (TZ_RANGE if self.mutant == "tz-second-run-96" else cdiv(TZ_RANGE, 2)):
                before = best_dist
                best_dist = self.tz_pattern(dist, sx, sy, best_dist)
                if best_dist == dist and (before != dist):
                    self.hit("tz:run2:improves")
                if best_dist != dist:
                    rounds += 1
                if rounds >= limit:
                    broke = True
                    break
                dist *= 2
            self.hit("tz:run2:break3" if broke else "tz:run2:to-end")
        else:
            self.hit("tz:run2:absent")
        loops = 0
        while best_dist > 0 and self.mutant != "tz-no-refinement" and not (self.mutant == "tz-refine-once" and loops == 1):
            loops += 1
            best_dist = 0
            sx, sy = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
            dist = 1
            while dist <= top:
                best_dist = self.tz_pattern(dist, sx, sy, best_dist)
                dist *= 2
        self.hit("tz:refine:%s" % ("2+" if loops >= 2 else loops))

    # ---- search_mv_full (:886-956)
    def window_sads(self, cx, cy):
        """the SADs of the (2R + 1)^2 positions around (cx, cy), [row][column], from a sliding-window view of the clamped reference"""
        R = self.range
        region = self.clamped(self.x + cx - R, self.y + cy - R, self.w + 2 * R, self.h + 2 * R).astype(np.int16)
        views = np.lib.stride_tricks.sliding_window_view(region, (self.h, self.w))
        cur = self.cur.astype(np.int16)
        out = np.empty((2 * R + 1, 2 * R + 1), np.int64)
        for r in range(2 * R + 1):
            out[r] = np.abs(views[r] - cur).sum(axis=(1, 2), dtype=np.int64)
        return out

    def full(self):
        R = self.range
        fits = window_fits(self.w, self.h, R)
        self.hit("full:lds:%d:%s" % ({1: 16, 2: 32, 4: 64}[size_class(self.w, self.h)], "fits" if fits else "no-fit"))
        won = None

        def window(cx, cy, name, skip=None):
            nonlocal won
            sads = self.window_sads(cx, cy)
            self.begin_group("full")
            count = 0
            for y in range(cy - R, cy + R + 1):
                x = cx - R
                while x <= cx + R:
                    if skip is not None:
                        if not self.within(x * 4, y * 4):              # :928-930
                            self.hit("full:within-false")
                            x += 1
                            continue
                        jump = skip(x, y)
                        if jump is not None:
                            x = jump + 1
                            continue
                    count += 1
                    if self.check(x, y, int(sads[y - (cy - R), x - (cx - R)])):
                        won = name
                    x += 1
            self.end_group()
            if count % ME_GROUP:
                self.hit("full:last-group-short")

        window(0, 0, "zero-window")
        ex, ey = asr(self.extra[0], 2), asr(self.extra[1], 2)
        if self.mutant == "full-extra-in-merge-searched":
            ex, ey = asr(self.extra[0] + 2, 2), asr(self.extra[1] + 2, 2)
        if not self.in_merge(asr(self.extra[0], 2), asr(self.extra[1], 2)):
            self.hit("full:extra:window")
            window(ex, ey, "extra-window")
        else:
            self.hit("full:extra:in-merge")
        shift = (lambda v: asr(v + 2, 2)) if self.mutant == "full-rounded-shift" else (lambda v: asr(v, 2))     # a plain shift here (:916-917)
        for i, (mx, my, usable, _) in enumerate(self.merge):
            if not usable:
                self.hit("full:merge%d:unusable" % i)
                continue
            cx, cy = shift(mx), shift(my)
            if cx == 0 and cy == 0:
                self.hit("full:merge%d:zero" % i)
                continue
            self.hit("full:merge%d:window" % i)

            def skip(x, y, i=i):
                """:933-950: inside the window of the zero vector or of an earlier candidate -> the last column of that window"""
                for j in range(-1, i):
                    xx = yy = 0
                    if j >= 0:
                        inside = lambda: (shift(self.merge[j][0]) - R <= x <= shift(self.merge[j][0]) + R and
                                          shift(self.merge[j][1]) - R <= y <= shift(self.merge[j][1]) + R)
                        if not self.merge[j][2]:
                            if inside():
                                self.hit("full:unusable-earlier-not-counted")
                            if self.mutant != "full-unusable-window-counted":
                                continue
                        xx, yy = shift(self.merge[j][0]), shift(self.merge[j][1])
                    if xx - R <= x <= xx + R and yy - R <= y <= yy + R:
                        self.hit("full:jump:%s" % ("zero-window" if j < 0 else "merge%d" % j))
                        return xx + R + (1 if self.mutant == "full-jump-plus-one" else 0)
                return None
            window(cx, cy, "merge-window", skip)
        if won:
            self.hit("full:winner:%s" % won)

    # ---- search_frac (:965-1128): the control flow; the filtered samples and their SATD are the oracle's
    def frac(self):
        mx, my = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
        w, h = self.w, self.h
        iw, ih = ((w + 7) >> 3) << 3, ((h + 7) >> 3) << 3                                   # :1000-1001
        # kvz_get_extended_block (:1008-1013): the block at mv - (1, 1), one pixel larger, with 4 pixels of filter margin on every side
        ext = np.ascontiguousarray(self.clamped(self.x + mx - 1 - 4, self.y + my - 1 - 4, iw + 1 + 8, ih + 1 + 8))
        es = ext.shape[1]
        cur = np.ascontiguousarray(self.pic[self.y:self.y + h, self.x:self.x + w])
        level = 4 if (self.mutant == "frac-level-as-4") else self.fme
        best_cost = int(O.satd_any_size(w, h, cur, 0, w, ext, 5 * es + 5, es))              # :1019-1021
        best_bits = self.bits(mx, my, 2)
        best_cost = (best_cost + self.price(best_bits)) & U32
        int_mx, int_my = mx, my
        mx, my = mx * 2, my * 2                                                             # half-pel (:1034-1035)
        best_index, i, off = 0, 1, (0, 0)
        filtered = O.filter_frac_steps(ext, 4, 4, iw, ih, (0, 0), level)
        for step in range(level):
            mv_shift = 1 if step < 2 else 0
            if step == 2:
                filtered = O.filter_frac_steps(ext, 4, 4, iw, ih, off, level)
            costs = [int(c) for c in O.satd_any_size_quad(w, h, [filtered[step][j] for j in range(4)], 64, cur, 0, w)]
            within, bits = [], [0] * 4
            self.group, self.g_inc, self.g_costs = "frac", best_cost, []
            for j in range(4):
                px, py = mx + SQUARE[i + j][0], my + SQUARE[i + j][1]
                ok = self.within(px * (1 << mv_shift), py * (1 << mv_shift))                # :1064-1068
                if not ok:
                    self.mute += 1
                    would = (costs[j] + self.price(self.bits(px, py, mv_shift))) & U32
                    self.mute -= 1
                    if would < best_cost:
                        self.hit("frac:refused-would-have-won")
                    if self.mutant == "frac-within-ignored":
                        ok = True
                within.append(ok)
                if ok:
                    bits[j] = 0 if self.mutant == "frac-no-bits" else self.bits(px, py, mv_shift)
                    costs[j] = (costs[j] + self.price(bits[j])) & U32
                    self.g_costs.append(costs[j])
            self.end_group()
            incumbent = best_cost
            for j in range(4):
                if not within[j]:
                    continue
                better = costs[j] < best_cost
                if costs[j] == best_cost:
                    if self.mutant == "frac-le":
                        better = True
                    elif self.mutant == "last-wins":
                        better = best_cost < incumbent
                    elif self.mutant == "le-incumbent":
                        better = best_cost == incumbent
                if better:
                    best_cost, best_bits, best_index = costs[j], bits[j], i + j
            i += 4
            if step == 1 or step == level - 1:                                              # :1105-1120
                if step >= 2:
                    self.hit("frac:qpel:win%d" % best_index)
                mx, my = mx + SQUARE[best_index][0], my + SQUARE[best_index][1]
                if step == min(level - 1, 1):
                    self.hit("frac:hpel:win%d" % best_index)
                    mx, my = mx * 2, my * 2                                                 # quarter-pel
                    off = SQUARE[best_index]
                    if self.mutant == "frac-qpel-around-integer":
                        mx, my, off = int_mx * 4, int_my * 4, (0, 0)
                    best_index, i = 0, 1
        self.best_mv, self.best_cost, self.best_bits = (mx, my), best_cost, best_bits

    # ---- ref_me_search_pu: the search, the gate of search_pu_inter_ref (:1236-1252) and its result (:1253-1273)
    def run(self):
        w, h = self.w, self.h
        for name, yes in (("8x8", (w, h) == (8, 8)), ("16x16", (w, h) == (16, 16)), ("32x32", (w, h) == (32, 32)), ("64x64", (w, h) == (64, 64)),
                          ("generic-small", size_class(w, h) == 1 and (w, h) not in ((8, 8), (16, 16))),
                          ("generic-medium", size_class(w, h) == 2 and (w, h) != (32, 32)),
                          ("generic-big", size_class(w, h) == 4 and (w, h) != (64, 64)), ("w4", w == 4), ("w12", w == 12),
                          ("segs-not-pow2", ((w // (4 if w & 4 else 8)) * h) & ((w // (4 if w & 4 else 8)) * h - 1) != 0),
                          ("big-amp", size_class(w, h) == 4 and (w in (16, 48) or h in (16, 48)))):
            if yes:
                self.hit("shape:" + name)
        if self.lam in (0, 1 << 20):
            self.hit("cost:lambda:%s" % ("0" if self.lam == 0 else "2^20"))
        self.best_cost = U32
        {0: self.hexagon, 1: self.diamond, 2: self.tz, 3: self.full}[self.alg]()
        if self.fme > 0:
            if self.best_cost == U32:
                self.hit("frac:skipped-no-start")
            self.hit("frac:gate:%s" % ("equal" if self.best_cost == self.cost_to_beat else "open" if self.best_cost < self.cost_to_beat else "closed"))
        gate = self.best_cost <= self.cost_to_beat if self.mutant == "gate-le" else self.best_cost < self.cost_to_beat
        if self.fme > 0 and gate:
            self.hit("frac:level%d" % self.fme)
            self.frac()
        elif self.best_cost < U32:                               # :1242-1248: the SATD of the integer vector and its bits
            self.hit("frac:level0")
            mx, my = asr(self.best_mv[0], 2), asr(self.best_mv[1], 2)
            blk = np.ascontiguousarray(self.clamped(self.x + mx, self.y + my, w, h))
            cur = np.ascontiguousarray(self.pic[self.y:self.y + h, self.x:self.x + w])
            self.best_cost = (int(O.satd_any_size(w, h, cur, 0, w, blk, 0, w)) + self.price(self.best_bits)) & U32
        self.mute += 1
        m = self.merge_match(*self.best_mv)
        self.mute -= 1
        merged = m >= 0
        self.hit("result:merged" if merged else "result:not-merged")
        mv_cand = 0
        if not merged:
            mv_cand = self.select_cand(self.best_mv[0], self.best_mv[1], False)[0]
            if self.rdo:
                if self.mutant == "rdo-select-first":
                    mv_cand = 0
                self.hit("rdo:select:%s" % ("same-cands" if self.cand[0] == self.cand[1] else "cand%d" % mv_cand))
        return (self.best_mv[0], self.best_mv[1], self.best_cost, self.best_bits, int(merged), m if merged else len(self.merge), mv_cand)


def search_pu(pic, ref, pu, prm, cabac=None, cost_to_beat=None, mutant=None, census=None, trace=None):
    """one PU -> (mv x, mv y, cost, bitcost, merged, merge_idx, mv_cand); census: a Counter to add to; trace: a list that receives every
    improvement of the search"""
    prm = np.ascontiguousarray(prm).reshape(-1)[0]
    return _Search(np.asarray(pic), np.asarray(ref), pu, prm, cabac, cost_to_beat, mutant, census, trace).run()


def search_pu_batch(pic, ref, pus, prm, cabac=None, cost_to_beat=None, mutant=None):
    """-> (ME_RESULT [count], census of the batch: the number of PUs that reached each class)"""
    out = np.zeros(len(pus), dtype=ME_RESULT)
    total = collections.Counter()
    for i in range(len(pus)):
        census = collections.Counter()
        try:
            r = search_pu(pic, ref, pus[i], prm, cabac, None if cost_to_beat is None else cost_to_beat[i], mutant, census)
        except Runaway:
            r = (MAX_INT, MAX_INT, 0, 0, 0, 0, 0)                # a result no search gives
        out[i]["mv"], out[i]["cost"], out[i]["bitcost"], out[i]["merged"], out[i]["merge_idx"], out[i]["mv_cand"] = r[:2], r[2], r[3], r[4], r[5], r[6]
        total.update(census.keys())
    return out, total

"""A plain model of the merge / AMVP candidate derivation: what ref_lib.inter_candidates returns for one PU -- the completed ME_PU record
and the five MERGE_CAND records -- written from the reference's inter.c (kvz_inter_get_mv_cand, kvz_inter_get_merge_cand and their
helpers, :546-1446) and search_inter.c:1143-1206, one PU at a time, in plain integers.  It is written from neither the kernel nor the
oracle.  TEST INFRASTRUCTURE.

derive() also returns a census: a Counter of the decision classes taken, counted once per PU (CLASSES).  MUTANTS are deliberate errors of the
kind a kernel author could make, one at a time (derive(..., mutant=name)): the directed cases (tests/inter_cand_directed_cases.py) have
to reach every class and to notice every mutant.

What the reference's state looks like here (oracle/ref_harness.c: ref_inter_candidates): lcu->cu is cut from the tile's SCU map `cus`,
so a neighbour is the record at its tile-relative position; a record that is not inter carries no motion; frame->ref->cu_arrays holds
`col` at ref_LX[0][0] and `ref_cus` at ref_idx, and where the two are one picture the array is `col`; the merge list starts zeroed.

Two classes that one could expect have no place in CLASSES, because the reference's code cannot reach them (UNREACHABLE): in a B slice
add_temporal_candidate answers for both lists or for neither (nothing in it depends on the list but the vector), and the pair loop's
`i >= candidates || j >= candidates` never fires, since idx < cutoff * (cutoff - 1) keeps both below cutoff.

Two errors that suggest themselves are no mutants here, because they change nothing: A0 allowed at y % 64 + height == 64, and B0
allowed across the LCU's right edge below row 0.  In both places the coding-order test that follows refuses the neighbour anyway (a PU
that ends on the LCU's bottom edge is a lower child at every level of is_a0_cand_coded; one that ends on its right edge below row 0
meets case 3 of is_b0_cand_coded), so the reference's edge tests are redundant with it and no input tells the two apart."""
import collections

import numpy as np

from patterns import ME_PU, MERGE_CAND

PAIR_I = (0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3)
PAIR_J = (1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2)

GROUPS = ("spatial", "temporal", "scaling", "amvp", "merge", "descriptor")

CLASSES = tuple(
    ["a0:left-edge", "a0:lcu-bottom", "a0:picture-bottom", "a0:not-inter", "a0:not-coded-yet", "a0:taken-inside", "a0:taken-left-lcu",
     "b0:top-edge", "b0:picture-right", "b0:lcu-right-below-row-0", "b0:not-inter", "b0:not-coded-yet", "b0:taken-inside", "b0:taken-above-lcu",
     "b0:taken-above-right-lcu"] +
    ["%s:%s" % (n, k) for n in ("a1", "b1", "b2") for k in ("outside", "intra", "not-set", "inter")] +
    ["a1:barred", "b1:barred", "neighbour:unused-l0-ignored", "neighbour:unused-l1-ignored"] +
    ["col:none:no-references", "col:none:empty-l0", "col:none:tmvp-off", "col:none:poc-1-amvp-only", "h:taken", "h:outside-right", "h:outside-below",
     "h:lcu-row-boundary", "h:not-inter", "c3:taken", "c3:not-inter-either", "col-list:future-reference", "col-list:low-delay-l0",
     "col-list:low-delay-l1", "col-list:other-list"] +
    ["scale:equal-distances", "scale:dc-min", "scale:dc-max", "scale:dn-min", "scale:dn-max", "scale:scale-min", "scale:scale-max", "scale:mv-min",
     "scale:mv-max", "scale:negative-product", "scale:nothing-clamped"] +
    ["amvp:list-0", "amvp:list-1", "amvp:no-list", "amvp:left:a0", "amvp:left:a1", "amvp:left:other-list", "amvp:left:a0-scaled",
     "amvp:left:a1-scaled", "amvp:left:none", "amvp:above:b0", "amvp:above:b1", "amvp:above:b2", "amvp:above:none", "amvp:above-scaled:b0",
     "amvp:above-scaled:b1", "amvp:above-scaled:b2", "amvp:above-scaled:beside-an-unscaled-one", "amvp:above-scaled:suppressed-by-left",
     "amvp:equal-pair-dropped", "amvp:temporal-added", "amvp:temporal-not-needed", "amvp:temporal-none", "amvp:zero-pad-0", "amvp:zero-pad-1",
     "amvp:zero-pad-2"] +
    ["merge:a1:taken", "merge:a1:absent", "merge:b1:taken", "merge:b1:absent", "merge:b1:same-as-a1", "merge:b0:taken", "merge:b0:absent",
     "merge:b0:same-as-b1", "merge:a0:taken", "merge:a0:absent", "merge:a0:same-as-a1", "merge:b2:taken", "merge:b2:absent", "merge:b2:same-as-a1",
     "merge:b2:same-as-b1", "merge:b2:skipped-at-four", "merge:temporal:p-slice", "merge:temporal:b-slice-both-lists", "merge:temporal:none",
     "merge:temporal:off"] +
    ["merge:pair-%d:taken" % k for k in range(12)] +
    ["merge:pair:missing-list", "merge:pair:same-picture-and-vector", "merge:pair:table-exhausted", "merge:pair:left-at-five", "merge:zero:none",
     "merge:zero:first", "merge:zero:counting-up", "merge:zero:capped", "merge:zero:b-slice-min", "merge:zero:b-slice-min-0"] +
    ["desc:bipred-unusable", "desc:same-ref-0", "desc:same-ref-1", "desc:l1-only-vector", "extra:from-l0", "extra:from-l1", "extra:centre-not-inter",
     "extra:no-ref-cus", "desc:tile-offset", "desc:no-tile-offset"])
UNREACHABLE = ("merge:temporal:b-slice-one-list", "merge:pair:index-reaches-n")


def census_classes():
    return list(CLASSES)


# name -> (group, description)
_MUTANTS = {
    "a0-picture-bottom-ignored": ("spatial", "A0 not tested against the picture's bottom edge"),
    "a0-coded-no-walk": ("spatial", "A0's coding-order test answers yes for a lower-left child instead of walking to its parent"),
    "b0-picture-right-ignored": ("spatial", "B0 not tested against the picture's right edge"),
    "b0-coded-above-right-sibling": ("spatial", "B0's coding-order test answers no for a lower-left child (its B0 lies in the coded upper-right one)"),
    "pad-bits-swapped": ("spatial", "pad bit 0 bars B1 and bit 1 bars A1"),
    "unused-list-kept": ("spatial", "a neighbour's unused list is copied into the merge list with its vector and reference"),
    "not-set-is-inter": ("spatial", "a neighbour is available unless it is intra (type 0 passes)"),
    "h-on-lcu-row": ("temporal", "H allowed on an LCU row boundary"),
    "c3-before-h": ("temporal", "C3 taken before H"),
    "no-other-list": ("temporal", "the 1 - l fallback for a collocated CU without the wanted list is missing"),
    "poc-1-also-merge": ("temporal", "poc > 1 also required for the merge list's temporal candidate"),
    "h-outside-le": ("temporal", "H allowed at x + w == picture width or y + h == picture height"),
    "col-list-ignores-future": ("temporal", "the collocated list is always the current one, also with a reference after the picture"),
    "temporal-in-picture-coordinates": ("temporal", "H and C3 are looked up at the tile's offset (the reference uses tile-relative positions)"),
    "h-off-the-16-grid": ("temporal", "H and C3 are read at their own SCU, not at the top-left SCU of their 16 x 16 block"),
    "div-floor": ("scaling", "the division by the collocated distance rounds down instead of towards zero"),
    "no-negative-term": ("scaling", "the + (product < 0) term of the vector's rounding is missing"),
    "scale-clamp-4095": ("scaling", "scale clamped at -4095 .. 4095"),
    "dist-clamp-127": ("scaling", "the distances clamped at -127 .. 127"),
    "mv-wraps": ("scaling", "the scaled vector wraps to 16 bits instead of being clamped"),
    "dn-not-clamped": ("scaling", "the collocated distance is not clamped"),
    "above-scaled-despite-left": ("amvp", "a scaled above candidate is tried although a left neighbour exists"),
    "above-scaled-only-alone": ("amvp", "a scaled above candidate is tried only where no unscaled one was found"),
    "amvp-no-other-list": ("amvp", "a neighbour's other list is not tried"),
    "amvp-index-not-picture": ("amvp", "the unscaled test compares reference indices instead of pictures"),
    "amvp-equal-kept": ("amvp", "two equal spatial candidates are both kept"),
    "amvp-a1-first": ("amvp", "A1 tried before A0"),
    "amvp-b1-first": ("amvp", "B1 tried before B0"),
    "amvp-unused-list-used": ("amvp", "a neighbour's list is used although mv_dir does not name it"),
    "list-1-first": ("amvp", "the searched picture is looked for in L1 before L0 at each index"),
    "dup-l0-fields-only": ("merge", "the duplicate test compares the list-0 fields whatever the direction"),
    "dup-ignores-reference": ("merge", "the duplicate test compares vectors only"),
    "b2-against-b0": ("merge", "B2 compared with A1 and B0"),
    "b0-against-a1": ("merge", "B0 compared with A1 instead of B1"),
    "b2-not-limited": ("merge", "B2 taken although four candidates are there"),
    "pair-reject-by-index": ("merge", "the pair rejection compares reference indices instead of pictures"),
    "zero-fill-gt": ("merge", "zero fill with zero_idx > num_ref - 1"),
    "zero-fill-b-all-refs": ("merge", "zero fill counts all references in a B slice instead of min(before, after)"),
    "same-ref-by-index": ("descriptor", "same_ref compares the list index with ref_idx instead of the picture"),
    "extra-mv-l0-always": ("descriptor", "extra_mv always from list 0"),
    "centre-without-tile-offset": ("descriptor", "the centre CU looked up without the tile offset"),
    "centre-top-left": ("descriptor", "extra_mv from the CU at the PU's top-left corner"),
    "l1-only-vector-from-l0": ("descriptor", "a list-1-only candidate's descriptor vector read from list 0"),
    "bipred-usable": ("descriptor", "a bi-predictive candidate marked usable with its list-0 vector"),
}
_MUTANTS.update(("pair-table-entry-%d" % k, ("merge", "entry %d of the pair table, (%d, %d), with its two indices swapped" % (k, PAIR_I[k], PAIR_J[k])))
                for k in range(12))
MUTANTS = {k: v[1] for k, v in _MUTANTS.items()}
MUTANT_GROUP = {k: v[0] for k, v in _MUTANTS.items()}


def c_div(a, b):
    """C's division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def int16(v):
    return ((v + 32768) & 0xffff) - 32768


class Cu:
    """one SCU record; what is not inter carries no motion (flat_to_cu)"""
    __slots__ = ("type", "dir", "mv", "ref")

    def __init__(self, type_, dir_, mv, ref):
        self.type = type_
        inter = type_ == 2
        self.dir = dir_ if inter else 0
        self.mv = ((mv[0][0], mv[0][1]), (mv[1][0], mv[1][1])) if inter else ((0, 0), (0, 0))
        self.ref = (ref[0], ref[1]) if inter else (0, 0)


_EMPTY = Cu(0, 0, ((0, 0), (0, 0)), (0, 0))
_CACHE = {}


class _Map:
    """the records of a map, made as they are asked for"""

    def __init__(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        self.fields = (a["type"].tolist(), a["mv_dir"].tolist(), a["mv"].tolist(), a["mv_ref"].tolist())
        self.made = {}

    def __getitem__(self, i):
        if i not in self.made:
            assert i >= 0, "a record before the map"
            self.made[i] = Cu(*(f[i] for f in self.fields))
        return self.made[i]


def _records(a):
    """a map as Cu records; a read-only map (the directed cases') is converted once and kept"""
    if a is None:
        return None
    if isinstance(a, np.ndarray) and not a.flags.writeable:
        if id(a) not in _CACHE:
            _CACHE[id(a)] = (a, _Map(a))
        return _CACHE[id(a)][1]
    return _Map(a)


class _Model:
    def __init__(self, params, cus, col, ref_cus, mutant):
        assert mutant is None or mutant in MUTANTS, mutant
        p = np.ascontiguousarray(params).reshape(-1)[0]
        g = lambda k: int(p[k])
        self.m = mutant
        self.poc, self.is_b, self.tmvp, self.num_refs = g("poc"), g("slice_is_b") != 0, g("tmvp_enable") != 0, g("num_refs")
        self.ref_pocs = [int(v) for v in p["ref_pocs"]]
        self.ref_LX = [[int(v) for v in p["ref_LX"][l]] for l in range(2)]
        self.LX_size = [int(v) for v in p["ref_LX_size"]]
        self.col_ref_pocs = [int(v) for v in p["col_ref_pocs"]]
        self.col_ref_LX = [[int(v) for v in p["col_ref_LX"][l]] for l in range(2)]
        self.pic_w, self.pic_h, self.in_w, self.in_h = g("pic_width"), g("pic_height"), g("in_width"), g("in_height")
        self.tile_x, self.tile_y, self.ref_idx = g("tile_x"), g("tile_y"), g("ref_idx")
        self.cus_stride, self.col_stride = g("cus_stride"), g("col_stride")
        for a, s in ((cus, self.cus_stride), (col, self.col_stride), (ref_cus, self.col_stride)):
            assert a is None or np.asarray(a).ndim == 1 or np.asarray(a).shape[-1] == s, "a map's width is its stride"
        self.cus, self.col = _records(cus), _records(col)
        self.ref_map = self.col if ref_cus is col else _records(ref_cus)
        self.has_ref_cus = ref_cus is not None
        # the picture that holds the searched reference's CUs: cu_arrays[ref_idx]; it is the collocated one where the two are one picture
        col_pic = self.ref_LX[0][0] if self.LX_size[0] else -1
        if self.has_ref_cus and self.ref_idx == col_pic and self.col is not None:
            self.ref_map = self.col
        self.hits = None

    def hit(self, k):
        assert k in _CLASS_SET or k in UNREACHABLE, k
        self.hits.add(k)

    # ---------------------------------------------------------------- spatial neighbours (inter.c:566-874)
    def a0_coded(self, x, y, w, h):
        size = min(w & ~(w - 1), h & ~(h - 1))
        if h != size:
            y = y + h - size
        while size < 64:
            parent = 2 * size
            idx = (x % parent != 0) + 2 * (y % parent != 0)
            if idx == 0:
                return True
            if idx == 1 or idx == 3:
                return False
            if self.m == "a0-coded-no-walk":
                return True
            y -= size
            size = parent
        return False

    def b0_coded(self, x, y, w, h):
        size = min(w & ~(w - 1), h & ~(h - 1))
        if w != size:
            x = x + w - size
        while size < 64:
            parent = 2 * size
            idx = (x % parent != 0) + 2 * (y % parent != 0)
            if idx == 0:
                return True
            if idx == 2:
                return self.m != "b0-coded-above-right-sibling"
            if idx == 3:
                return False
            x -= size
            size = parent
        return True

    def cur(self, x, y):
        """lcu->cu at a tile-relative position: the LCU's own SCUs, the row above, the column to the left, the corner, the top-right SCU"""
        return self.cus[(y >> 2) * self.cus_stride + (x >> 2)]

    def cleared(self, cu):
        """inter_clear_cu_unused: -> (dir, mv, ref) with the unused list zeroed and its reference 255"""
        mv, ref = [cu.mv[0], cu.mv[1]], [cu.ref[0], cu.ref[1]]
        for l in range(2):
            if cu.dir & (1 << l):
                continue
            if cu.mv[l] != (0, 0):
                self.hit("neighbour:unused-l%d-ignored" % l)
            if self.m != "unused-list-kept":
                mv[l], ref[l] = (0, 0), 255
        return (cu.dir, (mv[0], mv[1]), (ref[0], ref[1]), cu)

    def available(self, cu, name):
        if cu.type == 2 or (self.m == "not-set-is-inter" and cu.type == 0):
            if name:
                self.hit(name + ":inter")
            return True
        if name:
            self.hit(name + (":intra" if cu.type == 1 else ":not-set"))
        return False

    def spatial(self, x, y, w, h):
        """-> {name: (dir, mv, ref) or None}"""
        c = dict(a0=None, a1=None, b0=None, b1=None, b2=None)
        xl, yl = x & 63, y & 63
        if x != 0:
            a1 = self.cur(x - 1, y + h - 1)
            if self.available(a1, "a1"):
                c["a1"] = self.cleared(a1)
            if not yl + h < 64:
                self.hit("a0:lcu-bottom")
            elif not (y + h < self.pic_h or self.m == "a0-picture-bottom-ignored"):
                self.hit("a0:picture-bottom")
            else:
                a0 = self.cur(x - 1, y + h)
                if not self.available(a0, None):
                    self.hit("a0:not-inter")
                elif not self.a0_coded(x, y, w, h):
                    self.hit("a0:not-coded-yet")
                else:
                    self.hit("a0:taken-inside" if xl else "a0:taken-left-lcu")
                    c["a0"] = self.cleared(a0)
        else:
            self.hit("a0:left-edge")
            self.hit("a1:outside")
        if y != 0:
            b0 = None
            if x + w < self.pic_w or self.m == "b0-picture-right-ignored":
                if xl + w < 64 or yl == 0:
                    b0 = self.cur(x + w, y - 1)
                else:
                    self.hit("b0:lcu-right-below-row-0")
            else:
                self.hit("b0:picture-right")
            if b0 is not None:
                if not self.available(b0, None):
                    self.hit("b0:not-inter")
                elif not self.b0_coded(x, y, w, h):
                    self.hit("b0:not-coded-yet")
                else:
                    self.hit("b0:taken-inside" if yl else "b0:taken-above-lcu" if xl + w < 64 else "b0:taken-above-right-lcu")
                    c["b0"] = self.cleared(b0)
            b1 = self.cur(x + w - 1, y - 1)
            if self.available(b1, "b1"):
                c["b1"] = self.cleared(b1)
            if x != 0:
                b2 = self.cur(x - 1, y - 1)
                if self.available(b2, "b2"):
                    c["b2"] = self.cleared(b2)
            else:
                self.hit("b2:outside")
        else:
            self.hit("b0:top-edge")
            self.hit("b1:outside")
            self.hit("b2:outside")
        return c

    # ---------------------------------------------------------------- the collocated CU (inter.c:713-781)
    def temporal(self, x, y, w, h):
        """-> the collocated CU (H, else C3) or None.  x, y are tile-relative, as the reference passes them"""
        if not self.num_refs:
            self.hit("col:none:no-references")
            return None
        if not self.LX_size[0] > 0:
            self.hit("col:none:empty-l0")
            return None
        if self.m == "temporal-in-picture-coordinates":
            x, y = x + self.tile_x, y + self.tile_y
        grid = (lambda v: v) if self.m == "h-off-the-16-grid" else (lambda v: (v >> 4) << 4)
        at = lambda px, py: self.col[grid(px) // 4 + (grid(py) // 4) * self.col_stride] if self.col is not None else _EMPTY
        xb, yb = x + w, y + h
        le = self.m == "h-outside-le"
        hcu = None
        if not (xb < self.in_w or (le and xb == self.in_w)):
            self.hit("h:outside-right")
        elif not (yb < self.in_h or (le and yb == self.in_h)):
            self.hit("h:outside-below")
        elif yb % 64 == 0 and self.m != "h-on-lcu-row":
            self.hit("h:lcu-row-boundary")
        elif at(xb, yb).type != 2:
            self.hit("h:not-inter")
        else:
            hcu = at(xb, yb)
        xc, yc = x + w // 2, y + h // 2
        c3 = None
        if xc < self.in_w and yc < self.in_h and at(xc, yc).type == 2:
            c3 = at(xc, yc)
        if self.m == "c3-before-h":
            hcu, c3 = c3, hcu
        if hcu is not None:
            self.hit("h:taken")
            return hcu
        self.hit("c3:taken" if c3 is not None else "c3:not-inter-either")
        return c3

    # ---------------------------------------------------------------- POC scaling (inter.c:955-980)
    def scaled_mv(self, mv, scale):
        prod = scale * int16(mv)
        if prod < 0:
            self.hit("scale:negative-product")
        v = (prod + 127 + (1 if prod < 0 and self.m != "no-negative-term" else 0)) >> 8
        if v < -32768:
            self.hit("scale:mv-min")
        if v > 32767:
            self.hit("scale:mv-max")
        return int16(v) if self.m == "mv-wraps" else clip(-32768, 32767, v)

    def scale_pocs(self, cur_poc, cur_ref_poc, nb_poc, nb_ref_poc, mv):
        dc, dn = cur_poc - cur_ref_poc, nb_poc - nb_ref_poc
        if dc == dn:
            self.hit("scale:equal-distances")
            return mv
        assert dn != 0, "the reference divides by zero here"
        lo = -127 if self.m == "dist-clamp-127" else -128
        clamped = False
        for v, name in ((dc, "dc"), (dn, "dn")):
            if v < -128:
                self.hit("scale:%s-min" % name)
                clamped = True
            if v > 127:
                self.hit("scale:%s-max" % name)
                clamped = True
        dc = clip(lo, 127, dc)
        if self.m != "dn-not-clamped":
            dn = clip(lo, 127, dn)
        num = 0x4000 + (abs(dn) >> 1)
        scale = (dc * (num // dn if self.m == "div-floor" else c_div(num, dn)) + 32) >> 6
        if scale < -4096:
            self.hit("scale:scale-min")
            clamped = True
        if scale > 4095:
            self.hit("scale:scale-max")
            clamped = True
        scale = clip(-4095 if self.m == "scale-clamp-4095" else -4096, 4095, scale)
        out = (self.scaled_mv(mv[0], scale), self.scaled_mv(mv[1], scale))
        if not clamped and -32768 <= (scale * mv[0] + 127) >> 8 <= 32767 and -32768 <= (scale * mv[1] + 127) >> 8 <= 32767:
            self.hit("scale:nothing-clamped")
        return out

    def temporal_vector(self, current_ref, colocated, reflist):
        """add_temporal_candidate (inter.c:1011-1061) -> the vector or None"""
        if colocated is None or not self.LX_size[0] > 0:
            return None
        colocated_ref = self.ref_LX[0][0]
        col_list = reflist
        future = any(self.ref_pocs[i] > self.poc for i in range(self.num_refs))
        if future and self.m != "col-list-ignores-future":
            col_list = 1
            self.hit("col-list:future-reference")
        else:
            self.hit("col-list:low-delay-l%d" % reflist)
        if (colocated.dir & (col_list + 1)) == 0 and self.m != "no-other-list":
            col_list = 1 - col_list
            self.hit("col-list:other-list")
        return self.scale_pocs(self.poc, self.ref_pocs[current_ref], self.ref_pocs[colocated_ref],
                               self.col_ref_pocs[self.col_ref_LX[col_list][colocated.ref[col_list]]], colocated.mv[col_list])

    # ---------------------------------------------------------------- AMVP (inter.c:1063-1194)
    def mvp(self, cand, reflist, lx_idx, scaling):
        """add_mvp_candidate -> (vector, through the other list) or None"""
        if cand is None:
            return None
        cdir, mv, ref, raw = cand
        if self.m == "amvp-unused-list-used":
            cdir, mv, ref = 3, raw.mv, raw.ref
        for i in range(2):
            cand_list = reflist if i == 0 else 1 - reflist
            if i == 1 and self.m == "amvp-no-other-list":
                continue
            if (cdir & (1 << cand_list)) == 0:
                continue
            if scaling:
                return self.scale_pocs(self.poc, self.ref_pocs[self.ref_LX[reflist][lx_idx]], self.poc,
                                       self.ref_pocs[self.ref_LX[cand_list][ref[cand_list] & 15]], mv[cand_list]), i == 1
            same = ref[cand_list] == lx_idx if self.m == "amvp-index-not-picture" else \
                self.ref_LX[cand_list][ref[cand_list] & 15] == self.ref_LX[reflist][lx_idx]
            if same:
                return mv[cand_list], i == 1
        return None

    def amvp(self, x, y, w, h, c, reflist, lx_idx):
        a = [("a0", c["a0"]), ("a1", c["a1"])]
        b = [("b0", c["b0"]), ("b1", c["b1"]), ("b2", c["b2"])]
        if self.m == "amvp-a1-first":
            a.reverse()
        if self.m == "amvp-b1-first":
            b[0], b[1] = b[1], b[0]
        out = []
        for scaling in (False, True):
            if out:
                break
            for name, cand in a:
                got = self.mvp(cand, reflist, lx_idx, scaling)
                if got:
                    out.append(got[0])
                    self.hit("amvp:left:" + name + ("-scaled" if scaling else ""))
                    if got[1]:
                        self.hit("amvp:left:other-list")
                    break
        if not out:
            self.hit("amvp:left:none")
        b_candidates = 0
        for name, cand in b:
            got = self.mvp(cand, reflist, lx_idx, False)
            if got:
                out.append(got[0])
                b_candidates = 1
                self.hit("amvp:above:" + name)
                break
        unscaled_above = b_candidates
        if c["a0"] or c["a1"]:
            if any(cand for _, cand in b) and len(out) < 2:
                self.hit("amvp:above-scaled:suppressed-by-left")
            if self.m != "above-scaled-despite-left" or len(out) == 2:
                b_candidates = 1
            else:
                b_candidates = 0
        elif len(out) != 2:
            b_candidates = 0
        if self.m == "above-scaled-only-alone" and unscaled_above:
            b_candidates = 1
        scaled_above = False
        if not b_candidates:
            for name, cand in b:
                got = self.mvp(cand, reflist, lx_idx, True)
                if got:
                    out.append(got[0])
                    scaled_above = True
                    self.hit("amvp:above-scaled:" + name)
                    if unscaled_above:
                        self.hit("amvp:above-scaled:beside-an-unscaled-one")
                    break
        if not unscaled_above and not scaled_above:
            self.hit("amvp:above:none")
        assert len(out) <= 2
        if len(out) == 2 and out[0] == out[1] and self.m != "amvp-equal-kept":
            out.pop()
            self.hit("amvp:equal-pair-dropped")
        col = self.temporal(x, y, w, h)
        if not self.tmvp:
            self.hit("col:none:tmvp-off")
        elif not self.poc > 1:
            self.hit("col:none:poc-1-amvp-only")
        elif self.num_refs and len(out) == 2:
            self.hit("amvp:temporal-not-needed")
        if self.tmvp and self.poc > 1 and self.num_refs and len(out) < 2 and col is not None:
            v = self.temporal_vector(self.ref_LX[reflist][lx_idx], col, reflist)
            if v is not None:
                out.append(v)
                self.hit("amvp:temporal-added")
        elif len(out) < 2:
            self.hit("amvp:temporal-none")
        self.hit("amvp:zero-pad-%d" % (2 - len(out)))
        while len(out) < 2:
            out.append((0, 0))
        return out

    # ---------------------------------------------------------------- the merge list (inter.c:1262-1446)
    def duplicate(self, c1, c2):
        if c2 is None or c1[0] != c2[0]:
            return False
        for l in range(2):
            used = c1[0] & (1 << l)
            if self.m == "dup-l0-fields-only":
                used = l == 0
            if used and (c1[1][l] != c2[1][l] or (c1[2][l] != c2[2][l] and self.m != "dup-ignores-reference")):
                return False
        return True

    def merge(self, x, y, w, h, c, use_a1, use_b1):
        """-> five (dir, mv, ref) records; every record starts zeroed, and a step writes the fields the reference writes"""
        c = dict(c)
        if not use_a1:
            c["a1"] = None
            self.hit("a1:barred")
        if not use_b1:
            c["b1"] = None
            self.hit("b1:barred")
        out = [dict(dir=0, mv=[(0, 0), (0, 0)], ref=[0, 0]) for _ in range(5)]
        n = 0
        for name, others in (("a1", ()), ("b1", ("a1",)), ("b0", ("a1",) if self.m == "b0-against-a1" else ("b1",)), ("a0", ("a1",)),
                             ("b2", ("a1", "b0") if self.m == "b2-against-b0" else ("a1", "b1"))):
            if name == "b2" and n >= 4 and self.m != "b2-not-limited":
                self.hit("merge:b2:skipped-at-four")
                continue
            cand = c[name]
            if cand is None:
                self.hit("merge:%s:absent" % name)
                continue
            dup = [o for o in others if self.duplicate(cand, c[o])]
            if dup:
                if "merge:%s:same-as-%s" % (name, dup[0]) in _CLASS_SET:
                    self.hit("merge:%s:same-as-%s" % (name, dup[0]))
                continue
            self.hit("merge:%s:taken" % name)
            out[n] = dict(dir=cand[0], mv=[cand[1][0], cand[1][1]], ref=[cand[2][0], cand[2][1]])
            n += 1
        if self.tmvp and n < 5 and self.num_refs and not (self.m == "poc-1-also-merge" and self.poc <= 1):
            out[n]["dir"] = 0
            answered = 0
            for reflist in range(2 if self.is_b else 1):
                col = self.temporal(x, y, w, h)
                v = self.temporal_vector(self.ref_LX[reflist][0], col, reflist)
                if v is not None:
                    out[n]["mv"][reflist] = v
                    out[n]["ref"][reflist] = 0
                    out[n]["dir"] |= 1 << reflist
                    answered += 1
            if answered == 0:
                self.hit("merge:temporal:none")
            elif not self.is_b:
                self.hit("merge:temporal:p-slice")
            else:
                self.hit("merge:temporal:b-slice-both-lists" if answered == 2 else "merge:temporal:b-slice-one-list")
            if out[n]["dir"]:
                n += 1
        else:
            self.hit("merge:temporal:off")
            if not self.tmvp:
                self.hit("col:none:tmvp-off")
            elif not self.num_refs:
                self.hit("col:none:no-references")
        if n < 5 and self.is_b:
            pi, pj = list(PAIR_I), list(PAIR_J)
            if self.m and self.m.startswith("pair-table-entry-"):
                k = int(self.m.rsplit("-", 1)[1])
                pi[k], pj[k] = pj[k], pi[k]
            cutoff, idx = n, 0
            while True:
                if not idx < cutoff * (cutoff - 1):
                    self.hit("merge:pair:table-exhausted")
                    break
                if n == 5:
                    self.hit("merge:pair:left-at-five")
                    break
                i, j = pi[idx], pj[idx]
                if i >= n or j >= n:
                    self.hit("merge:pair:index-reaches-n")
                    break
                if (out[i]["dir"] & 1) and (out[j]["dir"] & 2):
                    out[n] = dict(dir=3, mv=[out[i]["mv"][0], out[j]["mv"][1]], ref=[out[i]["ref"][0], out[j]["ref"][1]])
                    if self.m == "pair-reject-by-index":
                        same_pic = out[i]["ref"][0] == out[j]["ref"][1]
                    else:
                        same_pic = self.ref_LX[0][out[i]["ref"][0] & 15] == self.ref_LX[1][out[j]["ref"][1] & 15]
                    if same_pic and out[i]["mv"][0] == out[j]["mv"][1]:
                        self.hit("merge:pair:same-picture-and-vector")
                    else:
                        self.hit("merge:pair-%d:taken" % idx)
                        n += 1
                else:
                    self.hit("merge:pair:missing-list")
                idx += 1
        num_ref = self.num_refs
        if n < 5 and self.is_b and self.m != "zero-fill-b-all-refs":
            before = sum(1 for j in range(self.num_refs) if self.ref_pocs[j] < self.poc)
            num_ref = min(before, self.num_refs - before)
            self.hit("merge:zero:b-slice-min" if num_ref else "merge:zero:b-slice-min-0")
        if n == 5:
            self.hit("merge:zero:none")
        zero_idx = 0
        while n != 5:
            capped = zero_idx > num_ref - 1 if self.m == "zero-fill-gt" else zero_idx >= num_ref - 1
            if zero_idx == 0:
                self.hit("merge:zero:first")
            elif capped:
                if num_ref > 1:
                    self.hit("merge:zero:capped")
            else:
                self.hit("merge:zero:counting-up")
            out[n]["mv"][0] = (0, 0)
            out[n]["ref"][0] = 0 if capped else zero_idx
            out[n]["ref"][1] = out[n]["ref"][0]
            out[n]["dir"] = 1
            if self.is_b:
                out[n]["mv"][1] = (0, 0)
                out[n]["dir"] = 3
            zero_idx += 1
            n += 1
        return out

    # ---------------------------------------------------------------- one PU (ref_inter_candidates; search_inter.c:1143-1206, :1470-1500)
    def find_list(self):
        for lx in range(max(self.LX_size)):
            order = (1, 0) if self.m == "list-1-first" else (0, 1)
            for l in order:
                if lx < self.LX_size[l] and self.ref_LX[l][lx] == self.ref_idx:
                    return l, lx
        return -1, 0

    def pu(self, x, y, w, h, pad):
        """-> (mv_cand, extra_mv, the descriptor's merge[] as (mv, usable, same_ref), the merge list as (dir, ref, mv), the classes taken)"""
        self.hits = set()
        x, y = x - self.tile_x, y - self.tile_y
        assert x >= 0 and y >= 0 and x + w <= self.pic_w and y + h <= self.pic_h and (x | y | w | h) & 3 == 0
        self.hit("desc:tile-offset" if self.tile_x or self.tile_y else "desc:no-tile-offset")
        bar_a1, bar_b1 = (pad & 2, pad & 1) if self.m == "pad-bits-swapped" else (pad & 1, pad & 2)
        c = self.spatial(x, y, w, h)
        merge = self.merge(x, y, w, h, c, not bar_a1, not bar_b1)
        desc = [((0, 0), 0, 0)] * 5
        for k, mc in enumerate(merge):
            d = mc["dir"]
            if d == 3:
                self.hit("desc:bipred-unusable")
                if self.m == "bipred-usable":
                    desc[k] = (mc["mv"][0], 1, 0)
                continue
            l = d - 1
            if l == 1:
                self.hit("desc:l1-only-vector")
            same = mc["ref"][l] == self.ref_idx if self.m == "same-ref-by-index" else self.ref_LX[l][mc["ref"][l] & 15] == self.ref_idx
            desc[k] = (mc["mv"][0 if self.m == "l1-only-vector-from-l0" else l], 1, int(same))
            self.hit("desc:same-ref-%d" % same)
        reflist, lx_idx = self.find_list()
        mv_cand = [(0, 0), (0, 0)]
        if reflist >= 0:
            self.hit("amvp:list-%d" % reflist)
            mv_cand = self.amvp(x, y, w, h, c, reflist, lx_idx)
        else:
            self.hit("amvp:no-list")
        extra = (0, 0)
        if not self.has_ref_cus:
            self.hit("extra:no-ref-cus")
        elif self.ref_idx < self.num_refs:                   # a picture of state->frame->ref; the harness leaves the vector zero otherwise
            ox, oy = (0, 0) if self.m == "centre-without-tile-offset" else (self.tile_x, self.tile_y)
            cx, cy = (x, y) if self.m == "centre-top-left" else (x + (w >> 1), y + (h >> 1))
            centre = self.ref_map[((oy + cy) >> 2) * self.col_stride + ((ox + cx) >> 2)]
            if centre.type == 2:
                l = 0 if (centre.dir & 1) or self.m == "extra-mv-l0-always" else 1
                self.hit("extra:from-l%d" % (0 if centre.dir & 1 else 1))
                extra = centre.mv[l]
            else:
                self.hit("extra:centre-not-inter")
        return mv_cand, extra, desc, [(mc["dir"], mc["ref"], mc["mv"]) for mc in merge], self.hits


_CLASS_SET = frozenset(CLASSES)


def derive(params, cus, col, ref_cus, pus, mutant=None):
    """-> (the completed ME_PU records, MERGE_CAND records [count, 5], census).  cus / col / ref_cus: 2-D CU_INFO maps as wide as
    cus_stride / col_stride (col and ref_cus may be None where ref_lib.inter_candidates allows it)"""
    md = _Model(params, cus, col, ref_cus, mutant)
    pus = np.ascontiguousarray(pus)
    out = pus.copy()
    merge_out = np.zeros((len(pus), 5), dtype=MERGE_CAND)
    census = collections.Counter()
    got = [md.pu(*g) for g in zip(*(pus[k].tolist() for k in ("x", "y", "width", "height", "pad")))]
    if got:
        out["num_merge_cand"] = 5
        out["mv_cand"], out["extra_mv"] = [g[0] for g in got], [g[1] for g in got]
        out["merge"]["mv"], out["merge"]["usable"], out["merge"]["same_ref"] = ([[d[k] for d in g[2]] for g in got] for k in range(3))
        merge_out["dir"], merge_out["ref"], merge_out["mv"] = ([[m[k] for m in g[3]] for g in got] for k in range(3))
    for g in got:
        census.update(g[4])
    return out, merge_out, census


assert len(set(CLASSES)) == len(CLASSES) and ME_PU.itemsize == 64

"""A plain model of the deblocking filter with a census of its decisions.  TEST INFRASTRUCTURE.

Pure numpy and Python integers: no import of the oracle, the compiled reference or the library, so that it is a third, independent
statement of src/filter.c beside them.  deblock() filters all vertical edges of the picture, then all horizontal edges, on the 8 x 8
luma grid in 4-line segments, and counts every decision it takes in a collections.Counter: the census.  A census key is
"<direction>:<class>" for luma and "<direction>:<plane>:chroma:<class>" for chroma, direction v (vertical edges) or h, plane u or v;
a count is a number of 4-line segments.  census_classes() lists the classes a set of pictures has to reach.

mutate names one deliberate error (MUTANTS): what a kernel could get wrong in that place.  The tests use the mutants to show that the
directed pictures (deblock_directed_cases.py) would notice each of them."""
import collections

import numpy as np

TC_TABLE = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5,
            6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24)
BETA_TABLE = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30,
              32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64)
CHROMA_SCALE = tuple(range(30)) + (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37) + tuple(range(38, 52))
assert len(TC_TABLE) == 54 and len(BETA_TABLE) == 52 and len(CHROMA_SCALE) == 58
# part modes 2Nx2N, 2NxN, Nx2N, NxN, 2NxnU, 2NxnD, nLx2N, nRx2N: the PUs' (x, y) offsets in quarters of the CU
PART_OFFSETS = (((0, 0),), ((0, 0), (0, 2)), ((0, 0), (2, 0)), ((0, 0), (2, 0), (0, 2), (2, 2)), ((0, 0), (0, 1)), ((0, 0), (0, 3)),
                ((0, 0), (1, 0)), ((0, 0), (3, 0)))
TRANSPOSED_PART = (0, 2, 1, 3, 6, 7, 4, 5)

MUTANTS = {
    "strong-no-clamp": "strong filter without the +-2 tc clamp",
    "weak-no-10tc": "weak filter without the 10 tc test",
    "weak-10tc-le": "the 10 tc test with <= in place of <",
    "p0q0-wrap": "p0 / q0 of the weak filter without the 0..255 clamp, stored modulo 256",
    "second-wrap": "the second samples of the weak filter without the 0..255 clamp, stored modulo 256",
    "second-tc": "tc instead of tc >> 1 for the second samples",
    "side-le": "<= in the side threshold",
    "dpdq-le": "<= in dp + dq < beta",
    "5tc-no-round": "5 tc >> 1 in place of (5 tc + 1) >> 1",
    "beta3-le": "<= in the beta >> 3 test",
    "tc-idx-no-bs": "tc index without the 2 (bs - 1) term",
    "clamp-50-52": "index clamps at 50 and 52",
    "no-lower-clamp": "no lower index clamp: a negative index counts from the table's end",
    "qp-avg-no-round": "edge QP average without the + 1",
    "chroma-no-delta-clamp": "chroma delta without the +-tc clamp",
    "chroma-wrap": "chroma pixel without the 0..255 clamp, stored modulo 256",
    "chroma-no-intra-test": "chroma filtered on edges without an intra CU",
    "chroma-tc-luma-qp": "chroma tc from the luma QP",
    "cross-uses-straight": "the cross-matched branch using the straight pairing",
    "same-pic-or": "or for and in the same-picture branch",
    "undefined-not-zeroed": "undefined vectors not zeroed",
    "pu-no-amp": "PU boundaries ignoring the AMP offsets",
    "cbf-on-pu-edge": "the cbf rule applied on a PU-only edge",
    "tile-filtered": "a tile boundary filtered",
}

LUMA_CLASSES = (
    "edge:none", "edge:tu", "edge:pu", "edge:pu-amp",
    "bs2:intra-p", "bs2:intra-q", "bs2:intra-both", "bs1:cbf", "bs1:mv-uni-same-list", "bs1:mv-uni-diff-lists", "bs1:ref-uni", "bs0:p-slice",
    "b:straight:bs0", "b:straight:bs1", "b:cross:bs0", "b:cross:bs1", "b:same:far-far", "b:same:far-near", "b:same:near-far",
    "b:same:near-near", "b:refs-differ", "b:uni-vs-bi", "b:undefined-nonzero",
    "qp:odd-sum", "beta-idx:clamp0", "beta-idx:clamp51", "tc-idx:clamp0", "tc-idx:clamp53", "beta:zero", "off:dpdq", "on:tc0",
    "strong:unclipped", "strong:clip+", "strong:clip-",
    "weak:2nd:pq", "weak:2nd:p", "weak:2nd:q", "weak:2nd:none", "weak:abandoned", "weak:delta-clipped", "weak:delta-unclipped",
    "weak:2nd-clipped", "weak:p0q0-clamp0", "weak:p0q0-clamp255", "weak:2nd-clamp0", "weak:2nd-clamp255",
    "tile:skipped")
H_ONLY_CLASSES = ("deferred:plain", "deferred:tile-boundary")
CHROMA_CLASSES = ("intra-p", "intra-q", "intra-both", "intra-none", "qp<30", "qp30-43", "qp>43", "delta-clipped", "delta-unclipped",
                  "clamp0", "clamp255", "tc0")


def census_classes():
    """every census key a set of pictures has to reach"""
    keys = []
    for d in "vh":
        keys += ["%s:%s" % (d, c) for c in LUMA_CLASSES + (H_ONLY_CLASSES if d == "h" else ())]
        keys += ["%s:%s:chroma:%s" % (d, p, c) for p in "uv" for c in CHROMA_CLASSES]
    return keys


def _clip(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def _far(a, b):
    return abs(a[0] - b[0]) >= 4 or abs(a[1] - b[1]) >= 4


class _Model:
    def __init__(self, y, u, v, cus, prm, col_bd, row_bd, mutate):
        assert mutate is None or mutate in MUTANTS, mutate
        p = np.asarray(prm).reshape(-1)[0]
        self.m = mutate
        self.beta_off, self.tc_off, self.qp, self.frame_qp = (int(p[k]) for k in ("beta_offset_div2", "tc_offset_div2", "qp", "frame_qp"))
        self.per_cu_qp, self.slice_b, self.chroma = (int(p[k]) for k in ("per_cu_qp", "slice_is_b", "chroma"))
        self.ref_lx = np.asarray(p["ref_LX"]).astype(np.int64).tolist()
        self.h, self.w = (int(n) for n in y.shape)
        assert self.h % 8 == 0 and self.w % 8 == 0 and cus.shape == (self.h // 4, self.w // 4)
        self.planes = [np.asarray(a).astype(np.int64).tolist() if a is not None and (k == 0 or self.chroma) else None
                       for k, a in enumerate((y, u, v))]
        c = np.asarray(cus)
        self.cu = {k: c[k].astype(np.int64).tolist() for k in ("type", "depth", "part_size", "tr_depth", "cbf_y", "mv_dir", "qp", "mv", "mv_ref")}
        self.col_starts = set(64 * int(b) for b in col_bd[1:-1]) if col_bd is not None else set()
        self.row_starts = set(64 * int(b) for b in row_bd[1:-1]) if row_bd is not None else set()
        self.census = collections.Counter()

    def at(self, field, x, y):
        return self.cu[field][y >> 2][x >> 2]

    # ---- is_tu_boundary || is_pu_boundary -> (kind or None, tu_boundary)
    def boundary(self, x, y, d):
        pos = y if d else x
        if pos & ((64 >> self.at("tr_depth", x, y)) - 1) == 0:
            return "tu", True
        cu_width = 64 >> self.at("depth", x, y)
        x_cu, y_cu = x & ~(cu_width - 1), y & ~(cu_width - 1)
        part = self.at("part_size", x_cu, y_cu) & 7
        if self.m == "pu-no-amp":
            part = (0, 1, 2, 3, 1, 1, 2, 2)[part]
        for off in PART_OFFSETS[part]:
            if (y_cu if d else x_cu) + off[d] * cu_width // 4 == pos:
                return ("pu-amp" if off[d] in (1, 3) else "pu"), False
        return None, False

    def edge_qp(self, x, y, d):
        if not self.per_cu_qp:
            return self.qp, False
        if d and y > 0:
            qp_p = self.at("qp", x, y - 1)
        elif not d and x > 0:
            qp_p = self.at("qp", x - 1, y)
        else:
            qp_p = self.frame_qp
        s = qp_p + self.at("qp", x, y)
        return (s + (0 if self.m == "qp-avg-no-round" else 1)) >> 1, bool(s & 1)

    def record(self, x, y):
        return {k: self.at(k, x, y) for k in ("type", "cbf_y", "mv_dir", "mv", "mv_ref")}

    # ---- the boundary strength, -> (bs, [census classes])
    def strength(self, p, q, tu_b):
        if q["type"] == 1 or p["type"] == 1:
            return 2, ["bs2:intra-" + ("both" if q["type"] == p["type"] else ("p" if p["type"] == 1 else "q"))]
        if (tu_b or self.m == "cbf-on-pu-edge") and (q["cbf_y"] or p["cbf_y"]):
            return 1, ["bs1:cbf"]
        if p["mv_dir"] != 3 and q["mv_dir"] != 3:
            lp, lq = (p["mv_dir"] - 1) & 1, (q["mv_dir"] - 1) & 1
            if _far(q["mv"][lq], p["mv"][lp]):
                return 1, ["bs1:mv-uni-same-list" if lp == lq else "bs1:mv-uni-diff-lists"]
            if q["mv_ref"][lq] != p["mv_ref"][lp]:
                return 1, ["bs1:ref-uni"]
        if not self.slice_b:
            return 0, ["bs0:p-slice"]
        zero = self.m != "undefined-not-zeroed"
        mvp = [p["mv"][l] if (p["mv_dir"] >> l) & 1 or not zero else [0, 0] for l in range(2)]
        mvq = [q["mv"][l] if (q["mv_dir"] >> l) & 1 or not zero else [0, 0] for l in range(2)]
        ref = lambda c, l: self.ref_lx[l][c["mv_ref"][l] & 15] if (c["mv_dir"] >> l) & 1 else -1
        rp0, rp1, rq0, rq1 = ref(p, 0), ref(p, 1), ref(q, 0), ref(q, 1)
        if not ((rp0 == rq0 and rp1 == rq1) or (rp0 == rq1 and rp1 == rq0)):
            return 1, ["b:uni-vs-bi" if (p["mv_dir"] == 3) != (q["mv_dir"] == 3) else "b:refs-differ"]
        tags = []
        if any(not (c["mv_dir"] >> l) & 1 and c["mv"][l] != [0, 0] for c in (p, q) for l in range(2)):
            tags.append("b:undefined-nonzero")
        straight = _far(mvq[0], mvp[0]) or _far(mvq[1], mvp[1])
        cross = _far(mvq[1], mvp[0]) or _far(mvq[0], mvp[1])
        if rp0 != rp1:
            if rp0 == rq0:
                bs = int(straight)
                tags.append("b:straight:bs%d" % bs)
            else:
                bs = int(straight if self.m == "cross-uses-straight" else cross)
                tags.append("b:cross:bs%d" % int(cross))
        else:
            bs = int((straight or cross) if self.m == "same-pic-or" else (straight and cross))
            tags.append("b:same:%s-%s" % ("far" if straight else "near", "far" if cross else "near"))
        return bs, tags

    def table(self, table, index, top):
        """the lookup with its index clamps -> (value, "clamp0" / "clamp<top>" / None)"""
        hi = top - 1 if self.m == "clamp-50-52" else top
        if index < 0:
            return (table[index] if self.m == "no-lower-clamp" else table[0]), "clamp0"
        if index > top:
            return table[hi], "clamp%d" % top
        return table[min(index, hi)], None

    # ---- one luma segment: b[i] = p3 .. q3 of line i; -> tags; b is filtered in place
    def luma_segment(self, b, beta, tc):
        m, tags = self.m, set()
        dp0, dq0 = abs(b[0][1] - 2 * b[0][2] + b[0][3]), abs(b[0][4] - 2 * b[0][5] + b[0][6])
        dp3, dq3 = abs(b[3][1] - 2 * b[3][2] + b[3][3]), abs(b[3][4] - 2 * b[3][5] + b[3][6])
        dp, dq = dp0 + dp3, dq0 + dq3
        if beta == 0:
            tags.add("beta:zero")
        if not (dp + dq <= beta if m == "dpdq-le" else dp + dq < beta):
            if beta > 0:
                tags.add("off:dpdq")
            return tags
        if tc == 0:
            tags.add("on:tc0")
        tc52 = (5 * tc) >> 1 if m == "5tc-no-round" else (5 * tc + 1) >> 1
        flat = lambda l: abs(l[0] - l[3]) + abs(l[4] - l[7])
        b3 = (lambda l: flat(l) <= (beta >> 3)) if m == "beta3-le" else (lambda l: flat(l) < (beta >> 3))
        sw = (2 * (dp0 + dq0) < (beta >> 2) and 2 * (dp3 + dq3) < (beta >> 2) and abs(b[0][3] - b[0][4]) < tc52 and
              abs(b[3][3] - b[3][4]) < tc52 and b3(b[0]) and b3(b[3]))
        side = (beta + (beta >> 1)) >> 3
        p_2nd, q_2nd = (dp <= side, dq <= side) if m == "side-le" else (dp < side, dq < side)
        if not sw:
            tags.add("weak:2nd:" + (("pq" if q_2nd else "p") if p_2nd else ("q" if q_2nd else "none")))
        clipped = False
        for l in b:
            m0, m1, m2, m3, m4, m5, m6, m7 = l
            if sw:
                raw = ((2 * m0 + 3 * m1 + m2 + m3 + m4 + 4) >> 3, (m1 + m2 + m3 + m4 + 2) >> 2, (m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4) >> 3,
                       (m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4) >> 3, (m3 + m4 + m5 + m6 + 2) >> 2, (m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4) >> 3)
                for k, val in enumerate(raw):
                    old = l[k + 1]
                    if val > old + 2 * tc:
                        tags.add("strong:clip+")
                        clipped = True
                    elif val < old - 2 * tc:
                        tags.add("strong:clip-")
                        clipped = True
                    l[k + 1] = val if m == "strong-no-clamp" else _clip(old - 2 * tc, old + 2 * tc, val)
                continue
            delta = (9 * (m4 - m3) - 3 * (m5 - m2) + 8) >> 4
            keep = abs(delta) <= tc * 10 if m == "weak-10tc-le" else abs(delta) < tc * 10
            if not keep:
                if tc > 0:
                    tags.add("weak:abandoned")
                if m != "weak-no-10tc":
                    continue
            tags.add("weak:delta-clipped" if abs(delta) > tc else "weak:delta-unclipped")
            delta = _clip(-tc, tc, delta)
            tc2 = tc if m == "second-tc" else tc >> 1

            def store(val, what, wrap):
                if val < 0:
                    tags.add("weak:%s-clamp0" % what)
                elif val > 255:
                    tags.add("weak:%s-clamp255" % what)
                return val & 255 if wrap else _clip(0, 255, val)

            l[3] = store(m3 + delta, "p0q0", m == "p0q0-wrap")
            l[4] = store(m4 - delta, "p0q0", m == "p0q0-wrap")
            for on, k, raw in ((p_2nd, 2, (((m1 + m3 + 1) >> 1) - m2 + delta) >> 1), (q_2nd, 5, (((m6 + m4 + 1) >> 1) - m5 - delta) >> 1)):
                if on:
                    if abs(raw) > tc >> 1:
                        tags.add("weak:2nd-clipped")
                    l[k] = store(l[k] + _clip(-tc2, tc2, raw), "2nd", m == "second-wrap")
        if sw and not clipped:
            tags.add("strong:unclipped")
        return tags

    def count(self, d, tags, plane=None):
        for t in tags:
            self.census["%s:%s" % ("vh"[d], t) if plane is None else "%s:%s:chroma:%s" % ("vh"[d], plane, t)] += 1

    def run_pass(self, d):
        Y = self.planes[0]
        for uy in range(0, self.h, 8):
            for ux in range(0, self.w, 8):
                if (d == 0 and ux == 0) or (d == 1 and uy == 0):
                    continue
                if (ux in self.col_starts) if d == 0 else (uy in self.row_starts):
                    self.count(d, ["tile:skipped", "tile:skipped"])
                    if self.m != "tile-filtered":
                        continue
                at_lcu_end = d == 1 and (ux + 8) % 64 == 0 and ux + 8 != self.w
                deferred = at_lcu_end and (ux + 8) not in self.col_starts
                for s in range(2):
                    fx = ux + 4 if deferred and s == 1 else ux
                    kind, tu_b = self.boundary(fx, uy, d)
                    # the second half of a horizontal edge in front of an LCU's right border: its flags and QP come from that half's
                    # own SCU (the reference filters it with the next LCU) unless a tile ends there
                    if at_lcu_end and s == 1 and (self.boundary(ux, uy, d)[0] or self.boundary(ux + 4, uy, d)[0]):
                        self.count(d, ["deferred:plain" if deferred else "deferred:tile-boundary"])
                    self.count(d, ["edge:" + (kind or "none")])
                    if not kind:
                        continue
                    sx, sy = (ux + 4 * s, uy) if d else (ux, uy + 4 * s)
                    bs, tags = self.strength(self.record(sx, sy - 1) if d else self.record(sx - 1, sy), self.record(sx, sy), tu_b)
                    self.count(d, tags)
                    if not bs:
                        continue
                    qp, odd = self.edge_qp(fx, uy, d)
                    if odd:
                        self.count(d, ["qp:odd-sum"])
                    beta, hit = self.table(BETA_TABLE, qp + (self.beta_off << 1), 51)
                    if hit:
                        self.count(d, ["beta-idx:" + hit])
                    tc, hit = self.table(TC_TABLE, qp + (0 if self.m == "tc-idx-no-bs" else 2 * (bs - 1)) + (self.tc_off << 1), 53)
                    if hit:
                        self.count(d, ["tc-idx:" + hit])
                    if d == 0:
                        b = [Y[sy + i][sx - 4:sx + 4] for i in range(4)]
                    else:
                        b = [[Y[sy - 4 + k][sx + i] for k in range(8)] for i in range(4)]
                    self.count(d, self.luma_segment(b, beta, tc))
                    for i in range(4):
                        if d == 0:
                            Y[sy + i][sx - 4:sx + 4] = b[i]
                        else:
                            for k in range(8):
                                Y[sy - 4 + k][sx + i] = b[i][k]
                if self.chroma and ((uy if d else ux) & 15) == 0:
                    self.chroma_unit(ux, uy, d)

    # ---- chroma: one 4-line segment of each plane per unit on the 8 x 8 chroma grid
    def chroma_unit(self, ux, uy, d):
        if not self.boundary(ux, uy, d)[0]:
            return
        tp, tq = (self.at("type", ux, uy - 2) if d else self.at("type", ux - 2, uy)), self.at("type", ux, uy)
        if tp != 1 and tq != 1:
            for plane in "uv":
                self.count(d, ["intra-none"], plane)
            if self.m != "chroma-no-intra-test":
                return
            who = None
        else:
            who = "intra-" + ("both" if tp == tq else ("p" if tp == 1 else "q"))
        qp = self.edge_qp(ux, uy, d)[0]
        qpc = qp if self.m == "chroma-tc-luma-qp" else CHROMA_SCALE[_clip(0, 57, qp)]
        tc = self.table(TC_TABLE, qpc + 2 + (self.tc_off << 1), 53)[0]
        xc, yc = ux >> 1, uy >> 1
        for plane, P in zip("uv", self.planes[1:]):
            tags = set([who] if who else [])
            tags.add("qp<30" if qp < 30 else ("qp30-43" if qp <= 43 else "qp>43"))
            if tc == 0:
                tags.add("tc0")
            for i in range(4):
                pos = [(yc + k, xc + i) for k in range(-2, 2)] if d else [(yc + i, xc + k) for k in range(-2, 2)]
                m2, m3, m4, m5 = (P[r][c] for r, c in pos)
                raw = (((m4 - m3) * 4) + m2 - m5 + 4) >> 3
                tags.add("delta-clipped" if abs(raw) > tc else "delta-unclipped")
                delta = raw if self.m == "chroma-no-delta-clamp" else _clip(-tc, tc, raw)
                for (r, c), val in ((pos[1], m3 + delta), (pos[2], m4 - delta)):
                    if val < 0:
                        tags.add("clamp0")
                    elif val > 255:
                        tags.add("clamp255")
                    P[r][c] = val & 255 if self.m == "chroma-wrap" else _clip(0, 255, val)
            if who:
                self.count(d, tags, plane)


def deblock(y, u, v, cus, prm, col_bd=None, row_bd=None, mutate=None):
    """-> ((y, u, v) filtered uint8 planes, u and v None without chroma; the census).  col_bd, row_bd: the tile boundaries in LCUs
    ([0, ..., LCU columns] / [0, ..., LCU rows]) of a tiled picture."""
    md = _Model(y, u, v, cus, prm, col_bd, row_bd, mutate)
    md.run_pass(0)
    md.run_pass(1)
    out = tuple(np.array(p, dtype=np.int64).astype(np.uint8) if p is not None else None for p in md.planes)
    return out, md.census

"""Test-side reference of kvz_hip_sao_stats_frame and kvz_hip_sao_frame, composed from the reference's own functions applied to
blocks blitted from the planes -- the compiled reference (ref_lib) where it was built, else the C restatement that the oracle tests
pin to it (oracle_lib).

Statistics: per LCU and plane the block of sao_search_luma / sao_search_chroma (sao.c:580-644) is blitted and handed to
calc_sao_edge_dir and calc_sao_bands.  ref_lib's harness has no entry for calc_sao_bands (a static function of sao.c), so the band
statistics always come from oracle_lib's restatement; tests/test_sao_frame_ref.py anchors them to the reference through
sao_band_ddistortion.  The candidates are a Python restatement of sao.c:188-240 and :368-397 with C's truncating division.

Reconstruction: per LCU rectangle the trimming of kvz_sao_reconstruct (sao.c:297-324), then sao_reconstruct_color; untouched pixels
are copied.  TEST INFRASTRUCTURE."""
import numpy as np

import oracle_lib as O
import patterns as P
import ref_lib as R

STATS = np.dtype([("edge", "<i4", (4, 2, 5)), ("band", "<i4", (2, 32))])
CAND = np.dtype([("edge_offsets", "<i4", (4, 5)), ("edge_ddist", "<i4", (4,)), ("band_offsets", "<i4", (4,)), ("band_position", "<i4"),
                 ("band_ddist", "<i4")])
EDGE_OFFSETS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))      # g_sao_edge_offsets (sao.h:58-63): (x, y) of a, b
EO_CAT = np.array([1, 2, 0, 3, 4])                                                                  # sao-generic.c:37
POISON_PIXEL, POISON_WORD = 0x5A, 0x5A5A5A5A
INT_MAX = 2 ** 31 - 1


def backend():
    return R if R.available() else O


def lcu_grid(width, height):
    return (width + 63) // 64, (height + 63) // 64


def lcu_blocks(width, height, color):
    """(x, y, w, h) of every LCU's block of the plane, raster order (sao.c:588-601, :620-632)"""
    sh = 1 if color else 0
    pw, ph, bs = width >> sh, height >> sh, 64 >> sh
    nx, ny = lcu_grid(width, height)
    return [(lx * bs, ly * bs, min(bs, pw - lx * bs), min(bs, ph - ly * bs)) for ly in range(ny) for lx in range(nx)]


def blit(plane, x, y, w, h):
    return np.ascontiguousarray(plane[y:y + h, x:x + w])


def compose_stats(src, rec, chroma=1, B=None):
    """-> STATS records [planes, LCUs]"""
    B = B or backend()
    height, width = src[0].shape
    n_planes = 3 if chroma else 1
    out = np.zeros((n_planes, len(lcu_blocks(width, height, 0))), dtype=STATS)
    for color in range(n_planes):
        for i, (x, y, w, h) in enumerate(lcu_blocks(width, height, color)):
            o, r = blit(src[color], x, y, w, h), blit(rec[color], x, y, w, h)
            for e in range(4):
                out[color, i]["edge"][e] = B.calc_sao_edge_dir(o, r, e, w, h)
            out[color, i]["band"] = O.calc_sao_bands(o, r, w, h)
    return out


def c_div(a, b):
    """C's integer division: truncation towards zero"""
    q = abs(int(a)) // abs(int(b))
    return q if (a < 0) == (b < 0) else -q


def clip(lo, hi, v):
    return max(lo, min(hi, v))


def edge_candidate(edge):
    """sao_search_edge_sao (sao.c:368-397) for one buffer, without the mode bits -> (offsets [4][5], ddist [4])"""
    offs, dd = np.zeros((4, 5), np.int32), np.zeros(4, np.int32)
    for e in range(4):
        total = 0
        for cat in range(1, 5):
            s, c = int(edge[e][0][cat]), int(edge[e][1][cat])
            o = 0
            if c != 0:
                o = clip(-7, 7, c_div(s + (c >> 1), c))
            if cat <= 2 and o < 0:
                o = 0
            if cat >= 3 and o > 0:
                o = 0
            offs[e, cat] = o
            total += c * o * o - 2 * o * s
        dd[e] = total
    return offs, dd


def band_candidate(band):
    """calc_sao_band_offsets (sao.c:188-240), line by line -- the comparison of :217 against a best_dist that is never updated included
    -> (offsets [4], band_position, ddist)"""
    dist, temp_offsets = [0] * 32, [0] * 32
    for b in range(32):
        best_dist = INT_MAX
        s, c = int(band[0][b]), int(band[1][b])
        offset = 0
        if c != 0:
            offset = clip(-7, 7, c_div(s + (c >> 1), c))
        dist[b] = 0 if offset == 0 else INT_MAX
        temp_offsets[b] = 0
        while offset != 0:
            temp_dist = c * offset * offset - 2 * offset * s
            if temp_dist < best_dist:
                dist[b] = temp_dist
                temp_offsets[b] = offset
            offset += -1 if offset > 0 else 1
    best_dist, pos = INT_MAX, 0
    for b in range(28):
        temp_dist = dist[b] + dist[b + 1] + dist[b + 2] + dist[b + 3]
        if temp_dist < best_dist:
            best_dist, pos = temp_dist, b
    return np.array(temp_offsets[pos:pos + 4], np.int32), pos, best_dist


def compose_cands(stats):
    out = np.zeros(stats.shape, dtype=CAND)
    for idx in np.ndindex(stats.shape):
        out[idx]["edge_offsets"], out[idx]["edge_ddist"] = edge_candidate(stats[idx]["edge"])
        out[idx]["band_offsets"], out[idx]["band_position"], out[idx]["band_ddist"] = band_candidate(stats[idx]["band"])
    return out


def effective(sao14, color):
    """the record as the entry applies it to a plane: (type, eo_class, band_position, offsets [5]), or None where it copies -- a type
    other than 1 / 2, an eo_class outside 0..3 of an edge record and a band position outside 0..31 of a band record are SAO_TYPE_NONE"""
    s = [int(v) for v in sao14]
    v = 1 if color == 2 else 0
    typ, cls, bp, offs = s[0], s[1], s[2 + v], s[4 + 5 * v:9 + 5 * v]
    if typ == 1 and 0 <= bp <= 31:
        return 1, cls, bp, offs
    if typ == 2 and 0 <= cls <= 3:
        return 2, cls, bp, offs
    return None


def trim(x, y, w, h, cls, pw, ph):
    """the row and column trimming of kvz_sao_reconstruct for an edge block (sao.c:297-324)"""
    (ax, ay), (bx, by) = EDGE_OFFSETS[cls]
    if x + w + ax > pw or x + w + bx > pw:
        w -= 1
    if x + ax < 0 or x + bx < 0:
        x, w = x + 1, w - 1
    if y + h + ay > ph or y + h + by > ph:
        h -= 1
    if y + ay < 0 or y + by < 0:
        y, h = y + 1, h - 1
    return x, y, w, h


def compose_recon(rec, sao_luma, sao_chroma, chroma=1, B=None):
    """-> (y, u, v): kvz_sao_reconstruct per LCU and plane on top of a copy of the deblocked planes"""
    B = B or backend()
    height, width = rec[0].shape
    out = []
    for color in range(3 if chroma else 1):
        plane = np.ascontiguousarray(rec[color], dtype=np.uint8)
        ph, pw = plane.shape
        dst = plane.copy()
        infos = sao_luma if color == 0 else sao_chroma
        for i, (x, y, w, h) in enumerate(lcu_blocks(width, height, color)):
            eff = effective(infos[i], color)
            if eff is None:
                continue
            if eff[0] == 2:
                x, y, w, h = trim(x, y, w, h, eff[1], pw, ph)
            if w > 0 and h > 0:
                dst[y:y + h, x:x + w] = B.sao_reconstruct_color(plane, x, y, w, h, infos[i], color)
        out.append(dst)
    return tuple(out + [None] * (3 - len(out)))


def direct_recon(rec, sao_luma, sao_chroma, chroma=1):
    """the per-pixel rule in numpy: the record of the pixel's own LCU, neighbours from the whole plane, unchanged where a neighbour
    lies outside"""
    height, width = rec[0].shape
    nx, _ = lcu_grid(width, height)
    out = []
    for color in range(3 if chroma else 1):
        plane = np.asarray(rec[color], dtype=np.int64)
        ph, pw = plane.shape
        sh = 6 - (1 if color else 0)
        yy, xx = np.mgrid[0:ph, 0:pw]
        lcu = (yy >> sh) * nx + (xx >> sh)
        infos = np.asarray(sao_luma if color == 0 else sao_chroma, dtype=np.int64)
        dst = plane.copy()
        pad = np.pad(plane, 1)
        for i in range(infos.shape[0]):
            eff = effective(infos[i], color)
            if eff is None:
                continue
            typ, cls, bp, offs = eff
            offs = np.array(offs)
            m = lcu == i
            if typ == 1:
                band = (plane >> 3) - bp
                hit = m & (band >= 0) & (band < 4)
                dst[hit] = np.clip(plane + np.where(hit, offs[np.clip(band, 0, 3) + 1], 0), 0, 255)[hit]
            else:
                (ax, ay), (bx, by) = EDGE_OFFSETS[cls]
                a = pad[1 + ay:1 + ay + ph, 1 + ax:1 + ax + pw]
                b = pad[1 + by:1 + by + ph, 1 + bx:1 + bx + pw]
                inside = ((xx + ax >= 0) & (xx + ax < pw) & (xx + bx >= 0) & (xx + bx < pw) & (yy + ay >= 0) & (yy + ay < ph) &
                          (yy + by >= 0) & (yy + by < ph))
                cat = EO_CAT[2 + np.sign(plane - a) + np.sign(plane - b)]
                hit = m & inside
                dst[hit] = np.clip(plane + offs[cat], 0, 255)[hit]
        out.append(dst.astype(np.uint8))
    return tuple(out + [None] * (3 - len(out)))


# ---- pictures ----
def make_planes(w, h, seed, chroma=1):
    """(src, rec), each (y, u, v): cells of 8 x 8 luma / 4 x 4 chroma pixels cut from the block kinds of patterns.sao_blocks (random,
    ramp, 0 / 255 extremes, rec == orig), rec = source + coding-like noise"""
    g = np.random.default_rng(seed)
    src, rec = [], []
    for k in range(3 if chroma else 1):
        pw, ph, cell = (w, h, 8) if k == 0 else (w // 2, h // 2, 4)
        o, r = P.sao_blocks(pw, ph, 6, seed + 10 * k)
        pick = g.integers(0, 6, (ph // cell + 1, pw // cell + 1))
        if pick.size <= 4:
            pick = 1 + pick % 4                                  # a picture of one cell: not the kind whose rec equals the source
        yy, xx = np.mgrid[0:ph, 0:pw]
        which = pick[yy // cell, xx // cell]
        src.append(np.ascontiguousarray(o.reshape(6, ph, pw)[which, yy, xx]))
        rec.append(np.ascontiguousarray(r.reshape(6, ph, pw)[which, yy, xx]))
    pad = [None] * (3 - len(src))
    return tuple(src + pad), tuple(rec + pad)


def make_records(w, h, seed, shift=0):
    """int32 [LCUs, 14]: type (lx + 2 ly + shift) % 3, so that horizontally and vertically adjacent LCUs differ; the edge LCUs walk through
    the four classes; offsets of both signs, up to +-7"""
    g = np.random.default_rng(seed)
    nx, ny = lcu_grid(w, h)
    s = np.zeros((nx * ny, 14), np.int32)
    edges = 0
    for ly in range(ny):
        for lx in range(nx):
            r = s[ly * nx + lx]
            r[0] = (lx + 2 * ly + shift) % 3
            r[1] = (edges + shift) % 4
            edges += r[0] == 2
            r[2:4] = g.integers(0, 29, 2)
            r[4:] = g.integers(-7, 8, 10)
            r[4] = r[9] = 0
    return s


# the pictures of tests/golden/sao_frame.npz: (name, width, height, chroma, seed)
FIXTURE_PICTURES = (("ragged", 200, 136, 1, 71), ("mono", 136, 72, 0, 72), ("one", 64, 64, 1, 73), ("tiny", 8, 8, 1, 74))


def fixture_case(name, w, h, chroma, seed):
    """-> (src, rec, sao_luma, sao_chroma)"""
    src, rec = make_planes(w, h, seed, chroma)
    luma, chro = make_records(w, h, seed + 1, 0), make_records(w, h, seed + 2, 1)
    if name == "ragged":
        # band windows at both ends of the range with offsets that leave it: clipping at 0 and at 255
        luma[1, 2], luma[1, 4:9] = 28, (0, 7, 6, 7, 7)
        luma[7, 2], luma[7, 4:9] = 0, (0, -7, -6, -7, -7)
        chro[0, 2:4], chro[0, 4:] = (0, 28), (0, -7, -7, -5, -7, 0, 7, 7, 5, 7)
    elif name == "mono":
        # malformed records: all of them copy
        luma[0, 0] = 3
        luma[1, 0:2] = (2, 7)
        luma[2, 0], luma[2, 2] = 1, 40
        luma[3, 0:2] = (2, -1)
        luma[4, 0], luma[4, 2] = 1, -3
        luma[5, 0:2] = (2, 1)
    elif name == "one":
        luma[0, 0:2] = (2, 3)
        chro[0, 0], chro[0, 2:4] = 1, (5, 40)              # U filtered, V malformed: a copy
    elif name == "tiny":
        luma[0, 0:2] = (2, 2)
        chro[0, 0:2] = (2, 0)
    return src, rec, luma, (chro if chroma else None)


def coverage(cases):
    """what the fixture must contain; cases: [(name, w, h, chroma, rec planes, sao_luma, sao_chroma)] -> list of what is missing"""
    types, classes, bps, malformed = set(), set(), set(), set()
    clip_lo = clip_hi = adjacent = False
    for (name, w, h, chroma, rec, luma, chro) in cases:
        nx, ny = lcu_grid(w, h)
        for color, infos in ((0, luma), (1, chro), (2, chro)):
            if infos is None:
                continue
            for i, s in enumerate(infos):
                eff = effective(s, color)
                if eff is None:
                    types.add(0)
                    if s[0] == 3:
                        malformed.add("type 3")
                    if s[0] == 2 and s[1] == 7:
                        malformed.add("eo_class 7")
                    if s[0] == 1 and s[2] == 40:
                        malformed.add("band_position 40")
                    continue
                types.add(eff[0])
                x, y, bw, bh = lcu_blocks(w, h, color)[i]
                blk = rec[color][y:y + bh, x:x + bw].astype(int)
                if eff[0] == 2:
                    classes.add(eff[1])
                    clip_lo |= bool((blk + min(eff[3]) < 0).any())
                    clip_hi |= bool((blk + max(eff[3]) > 255).any())
                else:
                    bps.add(eff[2])
                    for k in range(4):
                        inband = (blk >> 3) == eff[2] + k
                        clip_lo |= bool((blk[inband] + eff[3][1 + k] < 0).any())
                        clip_hi |= bool((blk[inband] + eff[3][1 + k] > 255).any())
        t = luma[:, 0].reshape(ny, nx)
        if nx > 1 and ny > 1:
            adjacent |= bool((t[:, 1:] != t[:, :-1]).all() and (t[1:] != t[:-1]).all())
    missing = ["type %d" % t for t in (0, 1, 2) if t not in types] + ["edge class %d" % c for c in range(4) if c not in classes]
    missing += [m for m in ("type 3", "eo_class 7", "band_position 40") if m not in malformed]
    for ok, what in ((28 in bps, "band position 28"), (clip_lo, "an offset that clips at 0"), (clip_hi, "an offset that clips at 255"),
                     (adjacent, "adjacent LCUs of different types")):
        if not ok:
            missing.append(what)
    return missing


def build_fixture(B=None):
    """numeric arrays only: per picture the source and deblocked planes, the SAO records, and the expected statistics, candidates (as
    int32 [planes * LCUs, 104 / 30]) and destination planes.  -> (dict, missing coverage)"""
    d, cases = {}, []
    for (name, w, h, chroma, seed) in FIXTURE_PICTURES:
        src, rec, luma, chro = fixture_case(name, w, h, chroma, seed)
        stats = compose_stats(src, rec, chroma, B)
        cands = compose_cands(stats)
        dst = compose_recon(rec, luma, chro, chroma, B)
        for k, n in enumerate("yuv"):
            if src[k] is not None:
                d["%s_src_%s" % (name, n)], d["%s_rec_%s" % (name, n)], d["%s_dst_%s" % (name, n)] = src[k], rec[k], dst[k]
        d[name + "_sao_luma"] = luma
        if chroma:
            d[name + "_sao_chroma"] = chro
        d[name + "_stats"] = stats.reshape(-1).view(np.int32).reshape(-1, 104)
        d[name + "_cands"] = cands.reshape(-1).view(np.int32).reshape(-1, 30)
        cases.append((name, w, h, chroma, rec, luma, chro))
    return d, coverage(cases)


def load_fixture_case(z, name, chroma):
    """-> (src, rec, sao_luma, sao_chroma, want) with want = {"stats", "cands", "dst"}"""
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    n_planes = 3 if chroma else 1
    want = {"stats": np.ascontiguousarray(z[name + "_stats"]).view(STATS).reshape(n_planes, -1),
            "cands": np.ascontiguousarray(z[name + "_cands"]).view(CAND).reshape(n_planes, -1), "dst": planes("dst")}
    return planes("src"), planes("rec"), z[name + "_sao_luma"], (z[name + "_sao_chroma"] if chroma else None), want


def pick_edge_records(cands, chroma=1):
    """a fixed policy for the chain test, NOT the reference's decision (which needs CABAC bit costs): per LCU the edge class of least
    edge_ddist if that is negative, else SAO_TYPE_NONE.  U and V share one record, so for chroma the class is chosen on the sum of
    their edge_ddist (the reference sums over both buffers) and each plane keeps its own offsets.  -> (sao_luma, sao_chroma) int32
    [LCUs, 14]"""
    n = cands.shape[1]
    luma, chro = np.zeros((n, 14), np.int32), np.zeros((n, 14), np.int32)
    for i in range(n):
        e = int(np.argmin(cands[0, i]["edge_ddist"]))
        if cands[0, i]["edge_ddist"][e] < 0:
            luma[i, 0:2], luma[i, 4:9] = (2, e), cands[0, i]["edge_offsets"][e]
        if chroma:
            dd = cands[1, i]["edge_ddist"].astype(np.int64) + cands[2, i]["edge_ddist"]
            e = int(np.argmin(dd))
            if dd[e] < 0:
                chro[i, 0:2], chro[i, 4:9], chro[i, 9:14] = (2, e), cands[1, i]["edge_offsets"][e], cands[2, i]["edge_offsets"][e]
    return luma, (chro if chroma else None)

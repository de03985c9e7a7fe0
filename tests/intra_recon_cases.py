"""Test-side reference of kvz_hip_intra_recon_frame: a Python walk of kvz_intra_recon_cu (intra.c:652-706) over a CU map in coding
order -- LCUs in raster order, z-order inside each -- which composes the expected reconstruction, coefficients, flags and cost inputs
TU by TU from the reference's own kvz_intra_build_reference, kvz_intra_predict and kvz_quantize_residual: the compiled reference
(ref_lib) where it was built, else the C restatement that the oracle tests pin to it (oracle_lib).  Every TU reads the planes as the
TUs before it left them.  TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import oracle_lib as O
import ref_lib as R
from patterns import CU_INFO

COST = RC.COST
POISON_MODE = 0xEE
SIZE_NXN = 3                                                         # cu.h: part_size_t


def backend():
    return R if R.available() else O


def intra_cus(cus, width, height):
    """(x, y, size) of every intra CU, the rule of RC.inter_cus with the type swapped"""
    seen = np.zeros(cus.shape, dtype=bool)
    typ, dep = cus["type"].astype(int), cus["depth"].astype(int)
    out = []
    for sy, sx in zip(*np.nonzero(typ == IC.CU_INTRA)):
        if seen[sy, sx] or dep[sy, sx] > 3:
            continue
        size = 64 >> dep[sy, sx]
        x, y = (4 * sx) & ~(size - 1), (4 * sy) & ~(size - 1)
        seen[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = True
        if x + size <= width and y + size <= height:
            out.append((int(x), int(y), int(size)))
    return out


def intra_mask(cus, width, height):
    """(luma, chroma, SCU) masks of the pixels / records of the intra CUs"""
    m = np.zeros((height, width), bool)
    for (x, y, s) in intra_cus(cus, width, height):
        m[y:y + s, x:x + s] = True
    return m, m[::2, ::2], m[::4, ::4]


def _zorder(ux, uy):
    return sum((((ux >> b) & 1) << (2 * b)) | (((uy >> b) & 1) << (2 * b + 1)) for b in range(4))


def scan_of(mode, leaf):
    """kvz_get_scan_order (encoderstate.c:1384-1398) of a TU whose luma leaf is `leaf` wide: depth >= 3 is leaf <= 8"""
    if leaf <= 8:
        if 6 <= mode <= 14:
            return 2
        if 22 <= mode <= 30:
            return 1
    return 0


def walk_tus(cus, modes, width, height, chroma=1):
    """-> [(plane, x, y, n, cu_x, cu_y, mode, scan, leaf)] in coding order; (x, y) in LUMA pixels, n the transform width, leaf the luma
    leaf's width.  The tree is that of RC.walk_tus; the mode of a luma TU is the luma byte at its own top-left SCU, that of a chroma
    TU the chroma byte at its luma top-left (transform.c:293-316, intra.c:694); a TU with a mode above 34 is left out."""
    trd = cus["tr_depth"].astype(int)
    starts = {(x, y): s for (x, y, s) in intra_cus(cus, width, height)}
    out = []

    def node(x, y, depth, cu):
        size = 64 >> depth
        if depth < 4 and (depth == 0 or trd[y // 4, x // 4] > depth):
            for dy in (0, size // 2):
                for dx in (0, size // 2):
                    node(x + dx, y + dy, depth + 1, cu)
            return
        m = int(modes[y // 4, x // 4, 0])
        if m <= 34:
            out.append((0, x, y, size) + cu + (m, scan_of(m, size), size))
        if chroma and (size > 4 or (x % 8 == 0 and y % 8 == 0)):
            m = int(modes[y // 4, x // 4, 1])
            if m <= 34:
                for p in (1, 2):
                    out.append((p, x, y, max(size // 2, 4)) + cu + (m, scan_of(m, size), size))
    order = sorted(range(256), key=lambda i: _zorder(i % 16, i // 16))
    for Y0 in range(0, height, 64):
        for X0 in range(0, width, 64):
            for i in order:
                x, y = X0 + 4 * (i % 16), Y0 + 4 * (i // 16)
                if (x, y) in starts:
                    node(x, y, {64: 0, 32: 1, 16: 2, 8: 3}[starts[(x, y)]], (x, y))
    return out


def build_ref(B, log2, color, plane, w, h, x, y):
    """kvz_intra_build_reference of the PU at luma (x, y) from the whole plane of `color` -> 130 bytes"""
    if B is R:
        return R.intra_build_reference_from_plane(log2, color, plane, w, h, x, y)
    return O.intra_build_reference_batch(log2, color, plane, w, h, [(x, y)])[0]


def predict(B, ref, log2, mode, color):
    """kvz_intra_predict with filter_boundary = luma (intra.c:603)"""
    luma = 1 if color == 0 else 0
    if B is R:
        return R.intra_predict(ref, log2, mode, color, luma)
    return O.intra_predict_batch(ref[None], log2, [mode], luma, luma)[0, 0]


def compose(src, rec, cus, modes, qp, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None):
    """the outputs of the entry: {"rec", "coeff", "cus", "cbf_out", "costs", "tus": [(plane, n, has, mode, scan, x, y, leaf, signhide)]}.
    rec: (y, u, v) planes as the inter stages left them (may be wider than the picture); init = RC.initial_outputs(...) (default
    zeros)."""
    B = B or backend()
    height, width = src[0].shape
    n_planes = 3 if chroma else 1
    full = [np.array(p, dtype=np.uint8) for p in rec[:n_planes]]
    work = [np.ascontiguousarray(p[:height >> (1 if k else 0), :width >> (1 if k else 0)]) for k, p in enumerate(full)]
    if init is None:
        n = ((width + 63) // 64) * ((height + 63) // 64)
        init = (tuple(np.zeros((n, 1024 if k else 4096), np.int16) if (k == 0 or chroma) else None for k in range(3)),
                np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, COST))
    coeff = [None if c is None else np.array(c) for c in init[0]]
    cbf_out, costs, cus = np.array(init[1]), np.array(init[2]), np.array(cus)
    lcus_x = (width + 63) // 64
    for (x, y, size) in intra_cus(cus, width, height):
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    summary = []
    for (p, x, y, n, cu_x, cu_y, mode, scan, leaf) in walk_tus(cus, modes, width, height, chroma):
        sh = 1 if p else 0
        log2 = {4: 2, 8: 3, 16: 4, 32: 5}[n]
        px, py = x >> sh, y >> sh
        ref = build_ref(B, log2, p, work[p], width, height, x, y)
        pred = predict(B, ref, log2, mode, p).reshape(n, n)
        s = src[p][py:py + n, px:px + n]
        r, c, has = B.quantize_residual_batch(s[None], pred[None], n, qp, p, scan, 1, slice_is_intra, signhide)
        r, c, has = r.reshape(n, n), c.reshape(-1), int(has[0] != 0)
        work[p][py:py + n, px:px + n] = r
        z = RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
        lcu = (y >> 6) * lcus_x + (x >> 6)
        coeff[p][lcu, z:z + n * n] = c
        span = (2 * n if p else n) // 4
        scu = (slice(y // 4, y // 4 + span), slice(x // 4, x // 4 + span))
        if p == 0:
            cus["cbf_y"][scu] = has
        cbf_out[scu] |= (has << p)
        d, dz = s.astype(np.int64) - r, s.astype(np.int64) - pred
        f = "_c" if p else "_y"
        costs["ssd" + f][cu_y // 4, cu_x // 4] += np.uint32((d * d).sum())
        costs["zero_ssd" + f][cu_y // 4, cu_x // 4] += np.uint32((dz * dz).sum())
        costs["coeff_abs" + f][cu_y // 4, cu_x // 4] += np.uint32(np.abs(c.astype(np.int64)).sum())
        summary.append((p, n, has, mode, scan, x, y, leaf, int(signhide)))
    for k in range(n_planes):
        full[k][:work[k].shape[0], :work[k].shape[1]] = work[k]
    pad = [None] * (3 - n_planes)
    return {"rec": tuple(full + pad), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": summary}


LISTED_MODES = (0, 1, 2, 10, 18, 26, 34, 8, 24)


def make_map(w, h, seed, intra_share=0.3, blank_share=0.1, deep_share=0.25, nxn_share=0.5, **kw):
    """RC.make_map with tr_depth and modes for the intra CUs -> (cus, ref_LX, modes [h / 4, w / 4, 2]).  An intra CU carries
    tr_depth = max(1, depth) (search_intra.c), an NxN 8x8 CU tr_depth 4 and four modes; a share of the CUs is split one or two levels
    deeper in the map alone.  The modes of other records are POISON_MODE.  intra_share 1: every CU intra."""
    cus, ref_LX = RC.make_map(w, h, seed, intra_share=intra_share, blank_share=blank_share, **kw)
    g = np.random.default_rng(seed + 11)
    modes = np.full(cus.shape + (2,), POISON_MODE, np.uint8)

    def pick():
        return int(LISTED_MODES[g.integers(0, len(LISTED_MODES))]) if g.random() < 0.6 else int(g.integers(0, 35))
    for (x, y, size) in intra_cus(cus, w, h):
        depth = {64: 0, 32: 1, 16: 2, 8: 3}[size]
        blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
        trd = max(1, depth)
        luma = pick()
        modes[blk + (0,)] = luma
        if size == 8 and g.random() < nxn_share:
            cus["part_size"][blk], trd = SIZE_NXN, 4
            four = g.permutation(np.array(LISTED_MODES))[:4] if g.random() < 0.7 else g.integers(0, 35, 4)
            modes[y // 4:y // 4 + 2, x // 4:x // 4 + 2, 0] = np.asarray(four, dtype=np.uint8).reshape(2, 2)
            luma = int(four[0])
        elif g.random() < deep_share:
            trd = min(4, trd + int(g.integers(1, 3)))
        cus["tr_depth"][blk] = trd
        # intra.mode_chroma: derived from luma or one of the four fixed candidates (search_intra.c)
        modes[blk + (1,)] = luma if g.random() < 0.5 else int((0, 26, 10, 1, 34)[g.integers(0, 5)])
    return cus, ref_LX, modes


def make_planes(cus, seed, chroma=1, pad=0, amps=(0, 0, 0, 1, 2, 4, 8, 16, 40)):
    """-> (src, rec): the source = a gentle gradient plus noise of one amplitude per 16x16 area (0 among them: TUs without
    coefficients); rec = what the inter stages left: the source plus a little noise outside the intra CUs, random bytes inside them
    (never read), `pad` extra columns of RC.POISON_PIXEL"""
    g = np.random.default_rng(seed)
    hs, ws = cus.shape
    h, w = 4 * hs, 4 * ws
    _, _, ms = intra_mask(cus, w, h)
    amp = np.kron(np.array(amps)[g.integers(0, len(amps), ((hs + 3) // 4, (ws + 3) // 4))], np.ones((4, 4), dtype=np.int64))[:hs, :ws]
    src, rec = [], []
    for k in range(3 if chroma else 1):
        u = 2 if k else 4
        ph, pw = hs * u, ws * u
        yy, xx = np.mgrid[0:ph, 0:pw]
        a = np.kron(amp, np.ones((u, u), dtype=np.int64))
        img = 60 + 40 * k + (xx * (3 + k) + yy * 2) // 8 + np.rint((g.random((ph, pw)) * 2 - 1) * a).astype(np.int64)
        s = np.clip(img, 0, 255).astype(np.uint8)
        inside = np.kron(ms, np.ones((u, u), dtype=bool))
        r = np.full((ph, pw + pad), RC.POISON_PIXEL, np.uint8)
        r[:, :pw] = np.where(inside, g.integers(0, 256, (ph, pw)), np.clip(s.astype(np.int64) + g.integers(-3, 4, (ph, pw)), 0, 255))
        src.append(s)
        rec.append(r)
    none = [None] * (0 if chroma else 2)
    return tuple(src + none), tuple(rec + none)


def poison_intra(rec, cus, seed, chroma=1):
    """the same planes with other random bytes inside the intra CUs"""
    g = np.random.default_rng(seed)
    hs, ws = cus.shape
    _, _, ms = intra_mask(cus, 4 * ws, 4 * hs)
    out = []
    for k in range(3 if chroma else 1):
        u = 2 if k else 4
        inside = np.kron(ms, np.ones((u, u), dtype=bool))
        r = np.array(rec[k])
        view = r[:inside.shape[0], :inside.shape[1]]
        view[inside] = g.integers(0, 256, int(inside.sum()))
        out.append(r)
    return tuple(out + [None] * (0 if chroma else 2))


# the pictures of tests/golden/intra_recon.npz: (name, width, height, chroma, qp, signhide, slice_is_intra, seed, intra_share)
FIXTURE_PICTURES = (("ragged", 200, 136, 1, 27, 1, 0, 61, 0.45), ("full", 256, 192, 1, 37, 1, 1, 62, 1.0), ("mono", 128, 128, 0, 27, 0, 0, 63, 0.5),
                    ("plain", 128, 64, 1, 37, 0, 1, 64, 0.6))


def fixture_case(name, w, h, chroma, qp, signhide, slice_is_intra, seed, intra_share):
    cus, _, modes = make_map(w, h, seed, intra_share=intra_share, blank_share=0.0 if intra_share == 1.0 else 0.1)
    src, rec = make_planes(cus, seed + 100, chroma)
    return src, rec, cus, modes


def coverage(tus, maps):
    """what a TU population (the "tus" of compose) and its maps [(cus, modes, w, h)] fail to exercise -> list"""
    missing = []
    luma = [t for t in tus if t[0] == 0]
    for n in (32, 16, 8, 4):
        if not any(t[1] == n for t in luma):
            missing.append("luma TU %d" % n)
    for leaf in (8, 4):
        if not any(t[0] == 1 and t[1] == 4 and t[7] == leaf for t in tus):
            missing.append("4x4 chroma TU under %dx%d luma" % (leaf, leaf))
    for n in (8, 4):
        for what, ok in (("planar", lambda m: m == 0), ("DC", lambda m: m == 1), ("2", lambda m: m == 2), ("10", lambda m: m == 10),
                         ("18", lambda m: m == 18), ("26", lambda m: m == 26), ("34", lambda m: m == 34), ("6..14", lambda m: 6 <= m <= 14 and m != 10),
                         ("22..30", lambda m: 22 <= m <= 30 and m != 26)):
            if not any(t[1] == n and t[8] and ok(t[3]) for t in luma):
                missing.append("mode %s on a luma TU of %d under signhide" % (what, n))
    for s in (1, 2):
        if not any(t[4] == s and t[2] and t[8] for t in tus if t[0] == 0) or not any(t[4] == s and t[8] for t in tus if t[0] > 0):
            missing.append("scan %d with sign hiding on luma and on chroma" % s)
    for p in range(3):
        for has in (0, 1):
            if not any(t[0] == p and t[2] == has for t in tus):
                missing.append("plane %d has_coeffs %d" % (p, has))
    nxn = diff = left = top = right = bottom = above_right = False
    at = 0
    for (cus, modes, w, h) in maps:
        for (x, y, s) in intra_cus(cus, w, h):
            m = modes[y // 4:(y + s) // 4, x // 4:(x + s) // 4]
            nxn |= s == 8 and cus[y // 4, x // 4]["part_size"] == SIZE_NXN and len(set(m[:, :, 0].reshape(-1).tolist())) == 4
            diff |= bool(m[0, 0, 0] != m[0, 0, 1])
        n_here = len(walk_tus(cus, modes, w, h, 1))
        for t in tus[at:at + n_here]:
            if t[0]:
                continue
            n, x, y = t[1], t[5], t[6]
            left |= x == 0
            top |= y == 0
            right |= x + n == w
            bottom |= y + n == h
            above_right |= y > 0 and y % 64 == 0 and x % 64 + 2 * n > 64 and x // 64 * 64 + 64 < w
        at += n_here
    for ok, what in ((nxn, "an NxN CU with four different modes"), (diff, "a chroma mode different from luma"), (left, "a TU at x = 0"),
                     (top, "a TU at y = 0"), (right, "a TU at the right edge"), (bottom, "a TU at the bottom edge"),
                     (above_right, "a TU whose references reach into the above-right LCU")):
        if not ok:
            missing.append(what)
    return missing


def build_fixture(B=None):
    """numeric arrays only: per picture the source and entry planes, the CU map (as bytes), the modes and, over poisoned outputs, the
    expected planes, coefficients, CU map, cbf_out and costs (as uint32 [.., 6]).  -> (dict, missing coverage)"""
    d, tus, maps = {}, [], []
    for pic in FIXTURE_PICTURES:
        name, w, h, chroma, qp, signhide, slice_is_intra = pic[:7]
        src, rec, cus, modes = fixture_case(*pic)
        want = compose(src, rec, cus, modes, qp, chroma, signhide, slice_is_intra, B=B, init=RC.initial_outputs(w, h, chroma))
        if chroma:
            tus += want["tus"]
            maps.append((cus, modes, w, h))
        for k, n in enumerate("yuv"):
            if src[k] is not None:
                d["%s_src_%s" % (name, n)], d["%s_in_%s" % (name, n)] = src[k], rec[k]
                d["%s_rec_%s" % (name, n)], d["%s_coeff_%s" % (name, n)] = want["rec"][k], want["coeff"][k]
        d[name + "_cus"] = cus.view(np.uint8).reshape(cus.shape + (20,))
        d[name + "_modes"] = modes
        d[name + "_cus_out"] = want["cus"].view(np.uint8).reshape(cus.shape + (20,))
        d[name + "_cbf_out"] = want["cbf_out"]
        d[name + "_costs"] = want["costs"].view(np.uint32).reshape(cus.shape + (6,))
        d[name + "_tus"] = np.array(want["tus"], dtype=np.int32).reshape(-1, 9)
    return d, coverage(tus, maps)


def load_fixture_case(z, name, chroma):
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    view = lambda a: np.ascontiguousarray(a).view(CU_INFO).reshape(a.shape[:2])
    want = {"rec": planes("rec"), "coeff": planes("coeff"), "cus": view(z[name + "_cus_out"]), "cbf_out": z[name + "_cbf_out"],
            "costs": np.ascontiguousarray(z[name + "_costs"]).view(COST).reshape(z[name + "_costs"].shape[:2])}
    return planes("src"), planes("in"), view(z[name + "_cus"]), z[name + "_modes"], want


assert_outputs_equal = RC.assert_outputs_equal

"""Test-side reference of the lossless entries of the picture chain: kvz_hip_inter_residual_frame_lossless and
kvz_hip_intra_recon_frame_lossless.

A Python walk composes the expected outputs TU by TU.  The trees are those of inter_residual_cases.walk_tus and
intra_recon_cases.walk_tus; the reference pixels and the prediction of an intra TU are the backend's own kvz_intra_build_reference and
kvz_intra_predict (ref_lib where the compiled reference was built, else oracle_lib), taken from the SOURCE plane: in the reference a
lossless picture's reconstruction is its source (encoderstate.c:1125-1127), so the walk needs no coding order.  Under a tile grid every
tile is a picture of its own (tile_chain_cases).  bypass() and rdpcm() are a few lines of numpy written from transform.c:73-123 --
those functions are static in the reference and have no harness entry -- and are pinned by known answers worked by hand and by the
decoder's side of DPCM (tests/test_lossless_ref.py).  TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import oracle_lib as O
import ref_lib as R
import tile_chain_cases as TC
from patterns import CU_INFO

COST = RC.COST
HOR, VER = 10, 26                                                    # the modes with DPCM (transform.c:362-368)


def backend():
    return R if R.available() else O


# ---------------------------------------------------------------- the arithmetic
def bypass(src, pred):
    """bypass_transquant (transform.c:73-100) -> (coeff int16 [n, n], rec, has_coeffs)"""
    c = (src.astype(np.int32) - pred.astype(np.int32)).astype(np.int16)
    return c, np.array(src, dtype=np.uint8), int(bool((c != 0).any()))


def rdpcm(coeff, mode):
    """rdpcm (transform.c:109-123): the walk from the bottom right makes every subtraction see the unmodified neighbour"""
    c = np.array(coeff, dtype=np.int16)
    n = c.shape[0]
    hor = mode == HOR
    for y in range(n - 1, -1 if hor else 0, -1):
        for x in range(n - 1, 0 if hor else -1, -1):
            c[y, x] -= c[y, x - 1] if hor else c[y - 1, x]
    return c


def decode(pred, coeff, mode, implicit_rdpcm):
    """the decoder's side: the running sum along the DPCM direction undoes it"""
    c = coeff.astype(np.int32)
    if implicit_rdpcm and mode in (HOR, VER):
        c = np.cumsum(c, axis=1 if mode == HOR else 0)
    return (pred.astype(np.int32) + c).astype(np.uint8)


def predict(B, ref, log2, mode, color, filter_boundary):
    """kvz_intra_predict with the filter_boundary of intra.c:621"""
    if B is R:
        return R.intra_predict(ref, log2, mode, color, int(filter_boundary))
    return O.intra_predict_batch(ref[None], log2, [mode], 1 if color == 0 else 0, int(filter_boundary))[0, 0]


# ---------------------------------------------------------------- the two stages
def _start(cus, width, height, chroma, init, owned):
    if init is None:
        n = ((width + 63) // 64) * ((height + 63) // 64)
        init = (tuple(np.zeros((n, 1024 if k else 4096), np.int16) if (k == 0 or chroma) else None for k in range(3)),
                np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, COST))
    coeff = [None if c is None else np.array(c) for c in init[0]]
    cbf_out, costs, cus = np.array(init[1]), np.array(init[2]), np.array(cus)
    for (x, y, size) in owned(cus, width, height):                   # the outputs that TUs accumulate into start from zero
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    return coeff, cbf_out, costs, cus


def _put(p, x, y, n, cu_x, cu_y, s, pred, c, has, rec, coeff, cus, cbf_out, costs, lcus_x):
    sh = 1 if p else 0
    rec[p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n] = s
    z = RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
    coeff[p][(y >> 6) * lcus_x + (x >> 6), z:z + n * n] = c.reshape(-1)
    span = (2 * n if p else n) // 4
    scu = (slice(y // 4, y // 4 + span), slice(x // 4, x // 4 + span))
    if p == 0:
        cus["cbf_y"][scu] = has
    cbf_out[scu] |= (has << p)
    dz = s.astype(np.int64) - pred
    f = "_c" if p else "_y"
    costs["zero_ssd" + f][cu_y // 4, cu_x // 4] += np.uint32((dz * dz).sum())
    costs["coeff_abs" + f][cu_y // 4, cu_x // 4] += np.uint32(np.abs(c.astype(np.int64)).sum())


def compose_inter(src, pred, cus, chroma=1, init=None):
    """kvz_hip_inter_residual_frame_lossless -> {"rec", "coeff", "cus", "cbf_out", "costs", "tus"}; pred may be wider than the picture"""
    height, width = src[0].shape
    n_planes = 3 if chroma else 1
    rec = [np.array(p, dtype=np.uint8) for p in pred[:n_planes]]
    coeff, cbf_out, costs, cus = _start(cus, width, height, chroma, init, RC.inter_cus)
    tus = []
    for (p, x, y, n, cu_x, cu_y) in RC.walk_tus(cus, width, height, chroma):
        sh = 1 if p else 0
        blk = (slice(y >> sh, (y >> sh) + n), slice(x >> sh, (x >> sh) + n))
        pr = np.array(rec[p][blk])
        c, s, has = bypass(src[p][blk], pr)
        _put(p, x, y, n, cu_x, cu_y, s, pr, c, has, rec, coeff, cus, cbf_out, costs, (width + 63) // 64)
        tus.append({"stage": 0, "plane": p, "n": n, "x": x, "y": y, "mode": -1, "leaf": 0, "has": has, "pred": pr.tobytes(),
                    "changed": False, "peak": int(np.abs(c.astype(np.int32)).max())})
    pad = [None] * (3 - n_planes)
    return {"rec": tuple(rec + pad), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": tus}


def compose_intra(src, rec, cus, modes, chroma=1, implicit_rdpcm=0, grid=None, B=None, init=None):
    """kvz_hip_intra_recon_frame_lossless; grid: (col_bd, row_bd) or None.  rec: the planes on entry -- only their pixels outside the
    intra TUs survive, none is read."""
    B = B or backend()
    height, width = src[0].shape
    n_planes = 3 if chroma else 1
    col_bd, row_bd = grid or TC.one_tile(width, height)
    out = [np.array(p, dtype=np.uint8) for p in rec[:n_planes]]
    coeff, cbf_out, costs, cus = _start(cus, width, height, chroma, init, XC.intra_cus)
    tus = []
    for t in TC.tiles(width, height, col_bd, row_bd):
        x0, y0, tw, th = t[0], t[1], t[2] - t[0], t[3] - t[1]
        sub_src = TC.crop_planes(src, t, n_planes)
        sub_cus, sub_modes = TC.crop_map(cus, t), TC.crop_map(modes, t)
        for (p, x, y, n, cu_x, cu_y, mode, _, leaf) in XC.walk_tus(sub_cus, sub_modes, tw, th, chroma):
            sh = 1 if p else 0
            log2 = {4: 2, 8: 3, 16: 4, 32: 5}[n]
            ref = XC.build_ref(B, log2, p, sub_src[p], tw, th, x, y)
            pr = predict(B, ref, log2, mode, p, p == 0 and not implicit_rdpcm).reshape(n, n)
            c, s, has = bypass(sub_src[p][y >> sh:(y >> sh) + n, x >> sh:(x >> sh) + n], pr)
            stored = rdpcm(c, mode) if implicit_rdpcm and mode in (HOR, VER) else c
            _put(p, x + x0, y + y0, n, cu_x + x0, cu_y + y0, s, pr, stored, has, out, coeff, cus, cbf_out, costs, (width + 63) // 64)
            tus.append({"stage": 1, "plane": p, "n": n, "x": x + x0, "y": y + y0, "mode": mode, "leaf": leaf, "has": has, "pred": pr.tobytes(),
                        "changed": bool((stored != c).any()), "peak": int(np.abs(stored.astype(np.int32)).max()),
                        "peak_d": int(np.abs((stored[:, 1:] if mode == HOR else stored[1:]).astype(np.int32)).max())})
    pad = [None] * (3 - n_planes)
    return {"rec": tuple(out + pad), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": tus}


def compose(case, implicit_rdpcm=0, B=None, grid="case", init=None):
    """-> (mid, full): the inter entry over `init` (default RC.initial_outputs: poison), then the intra entry on what it left"""
    w, h, chroma = case["width"], case["height"], case["chroma"]
    if grid == "case":
        grid = case["grid"]
    mid = compose_inter(case["src"], case["pred"], case["cus"], chroma, init or RC.initial_outputs(w, h, chroma))
    full = compose_intra(case["src"], mid["rec"], mid["cus"], case["modes"], chroma, implicit_rdpcm, grid, B,
                         (mid["coeff"], mid["cbf_out"], mid["costs"]))
    return mid, full


# ---------------------------------------------------------------- the pictures of tests/golden/lossless.npz
LUMA_MODES = (HOR, VER, HOR, VER, 0, 1, 1, 2, 18, 34, 9, 27)
TILED = ((0, 1, 2, 3), (0, 1, 2))                                    # 3 x 2 LCUs, every LCU a tile
# (name, width, height, chroma, seed, intra_share, grid or None, the implicit_rdpcm values recorded for the intra stage)
FIXTURE_PICTURES = (
    ("inter", 72, 72, 1, 811, 0.0, None, ()),
    ("intra", 72, 72, 1, 812, 1.0, None, (0, 1)),
    ("mono", 72, 72, 0, 813, 0.5, None, (1,)),
    ("mixed", 136, 72, 1, 814, 0.6, TILED, (0, 1)),
)
BAD_MODE = 0x40


def make_map(w, h, seed, intra_share):
    """every 32x32 area that fits: one CU with a 32x32 TU, or per 16x16 area one CU with a 16x16 TU or four 8x8 CUs, each with one 8x8
    TU or four 4x4 luma TUs (intra: NxN with four modes) and one 4x4 TU per chroma plane; the ragged strips hold the 8x8 CUs that
    fit.  The first 32x32 areas take the sizes in turn, so that a 72x72 picture holds them all.  Then the records the entries must skip:
    a 32x32 CU record in the ragged bottom strip, which would leave the picture, and modes above 34.  -> (cus, modes)"""
    g = np.random.default_rng(seed)
    cus = np.zeros((h // 4, w // 4), CU_INFO)
    modes = np.full(cus.shape + (2,), XC.POISON_MODE, np.uint8)
    turn, big = [0], [0]

    def cu(x, y, size, trd):
        blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
        intra = g.random() < intra_share
        cus["depth"][blk], cus["tr_depth"][blk] = {32: 1, 16: 2, 8: 3}[size], trd
        cus["type"][blk], cus["mv_dir"][blk] = (IC.CU_INTRA, 0) if intra else (IC.CU_INTER, 1)
        if intra:
            m = np.full((size // 4, size // 4), g.choice(LUMA_MODES))
            if size == 32:                                           # few of them fit: they take the two DPCM modes in turn
                m[:], big[0] = (HOR, VER)[big[0] % 2], big[0] + 1
            if trd == 4:
                cus["part_size"][blk] = XC.SIZE_NXN
                m = g.permutation(np.array(LUMA_MODES[2:]))[:4].reshape(2, 2)
            modes[blk + (0,)] = m
            modes[blk + (1,)] = int(m[0, 0]) if g.random() < 0.4 else int(g.choice((0, VER, HOR, 1, 34, VER, HOR)))

    def eights(x, y):
        for dy in (0, 8):
            for dx in (0, 8):
                if x + dx + 8 <= w and y + dy + 8 <= h:
                    cu(x + dx, y + dy, 8, 4 if g.random() < 0.6 else 3)

    for y in range(0, h, 32):
        for x in range(0, w, 32):
            fits = x + 32 <= w and y + 32 <= h
            kind = turn[0] % 4 if fits else 3
            turn[0] += fits
            if kind in (0, 2) and fits:
                cu(x, y, 32, 1)
                continue
            for dy in (0, 16):
                for dx in (0, 16):
                    if kind == 1 and g.random() < 0.75 and x + dx + 16 <= w and y + dy + 16 <= h:
                        cu(x + dx, y + dy, 16, 2)
                    else:
                        eights(x + dx, y + dy)
    if h % 32:
        blk = cus[(h - h % 32) // 4:, 0:8]
        blk["type"], blk["depth"], blk["tr_depth"], blk["mv_dir"] = (IC.CU_INTRA if intra_share == 1.0 else IC.CU_INTER), 1, 1, 1
        modes[(h - h % 32) // 4:, 0:8] = 1
    intra = XC.intra_cus(cus, w, h)
    if intra:
        (x, y, s), (x2, y2, s2) = intra[len(intra) // 2], intra[len(intra) // 3]
        modes[y // 4:(y + s) // 4, x // 4:(x + s) // 4, 0] = BAD_MODE
        modes[y2 // 4:(y2 + s2) // 4, x2 // 4:(x2 + s2) // 4, 1] = 35
    return cus, modes


def make_planes(w, h, seed, chroma):
    """-> (src, pred).  The source: a gradient with gentle noise; a flat rectangle (intra TUs inside it predict it exactly: cbf 0); a
    rectangle of random 0 / 255 pixels (DPCM of it passes +-255).  The prediction of the inter stage: the source plus noise of one
    amplitude per 16x16 area, 0 among them (pred == src: cbf 0)."""
    g = np.random.default_rng(seed)
    amp = np.kron(g.choice((0, 0, 1, 3, 10, 60), ((h + 15) // 16, (w + 15) // 16)), np.ones((16, 16), np.int64))[:h, :w]
    src, pred = [], []
    for k in range(3 if chroma else 1):
        u = 2 if k else 1
        ph, pw = h // u, w // u
        yy, xx = np.mgrid[0:ph, 0:pw]
        img = 70 + 30 * k + (xx * (5 + k) + yy * 3) // 4 + g.integers(-4, 5, (ph, pw))
        img[24 // u:64 // u, 0:28 // u] = 90 + 20 * k                             # flat
        loud = g.integers(0, 2, (ph, pw)) * 255
        img[0:24 // u, 36 // u:64 // u] = loud[0:24 // u, 36 // u:64 // u]
        img[40 // u:ph, 44 // u:pw] = loud[40 // u:ph, 44 // u:pw]
        s = np.clip(img, 0, 255).astype(np.uint8)
        a = amp[::u, ::u][:ph, :pw]
        noise = np.rint((g.random((ph, pw)) * 2 - 1) * a).astype(np.int64)
        src.append(s)
        pred.append(np.clip(s.astype(np.int64) + noise, 0, 255).astype(np.uint8))
    none = [None] * (0 if chroma else 2)
    return tuple(src + none), tuple(pred + none)


def fixture_case(pic):
    name, w, h, chroma, seed, share, grid, rdpcm = pic
    cus, modes = make_map(w, h, seed, share)
    src, pred = make_planes(w, h, seed + 100, chroma)
    return {"name": name, "width": w, "height": h, "chroma": chroma, "grid": grid, "rdpcm": rdpcm, "src": src, "pred": pred, "cus": cus, "modes": modes}


def coverage(runs):
    """what the fixture fails to exercise -> list.  runs: [(case, {implicit_rdpcm: (mid, full)}, {implicit_rdpcm: untiled full or None})]"""
    missing = []
    tus, maps = [], []
    for case, by, _ in runs:
        first = by[sorted(by)[0]]
        tus += first[0]["tus"]
        for r in sorted(by):
            tus += [dict(t, rdpcm=r) for t in by[r][1]["tus"]]
        maps.append(case)
    chroma_tus = [t for case, by, _ in runs if case["chroma"] for r in by for t in by[r][1]["tus"] + by[r][0]["tus"]]
    for stage, what in ((0, "inter"), (1, "intra")):
        for p, sizes in ((0, (4, 8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
            for n in sizes:
                if not any(t["stage"] == stage and t["plane"] == p and t["n"] == n for t in tus):
                    missing.append("%s: plane %d TU %d" % (what, p, n))
        if not any(t["stage"] == stage and t["has"] == 0 for t in tus):
            missing.append("%s: a TU with an all-zero residual" % what)
    dp = [t for t in tus if t["stage"] == 1 and t.get("rdpcm")]
    for m in (HOR, VER):
        for n in (4, 8, 16, 32):
            if not any(t["plane"] == 0 and t["n"] == n and t["mode"] == m for t in dp):
                missing.append("luma mode %d on a TU of %d under implicit_rdpcm" % (m, n))
        if not any(t["plane"] > 0 and t["mode"] == m for t in dp):
            missing.append("chroma mode %d under implicit_rdpcm" % m)
        if not any(t["mode"] == m and t["changed"] for t in dp):
            missing.append("a mode-%d TU whose stored coefficients differ from the plain residual" % m)
    # A stored |coeff| ABOVE 255 cannot come out of a real TU: modes 10 and 26 copy one reference pixel along the DPCM direction and
    # the boundary filter is off under implicit_rdpcm (intra.c:621), so a value that DPCM changed is the difference of two neighbouring
    # SOURCE pixels (test_lossless_ref.py holds every DPCM TU of the fixture to that).  The fixture must reach that bound; values beyond
    # it are a matter of rdpcm() alone and are pinned by the known answers.
    if not any(t["mode"] in (HOR, VER) and t["peak_d"] == 255 for t in dp):
        missing.append("a stored |coeff| of 255 made by DPCM")
    if not any(t["plane"] > 0 and t["n"] == 4 and t["leaf"] == 4 for t in chroma_tus):
        missing.append("a 4x4 chroma TU under 4x4 luma TUs")
    nxn = ragged_r = ragged_b = edge = bad_l = bad_c = False
    for case in maps:
        cus, modes, w, h = case["cus"], case["modes"], case["width"], case["height"]
        for (x, y, s) in XC.intra_cus(cus, w, h):
            m = modes[y // 4:(y + s) // 4, x // 4:(x + s) // 4]
            nxn |= bool(case["chroma"] and s == 8 and cus[y // 4, x // 4]["tr_depth"] == 4 and len(set(m[:, :, 0].reshape(-1).tolist())) == 4
                        and m[0, 0, 1] <= 34)
            bad_l |= bool(m[0, 0, 0] > 34)
            bad_c |= bool(case["chroma"] and m[0, 0, 1] > 34)
        kept = np.zeros(cus.shape, bool)
        for (x, y, s) in XC.intra_cus(cus, w, h) + RC.inter_cus(cus, w, h):
            kept[y // 4:(y + s) // 4, x // 4:(x + s) // 4] = True
            ragged_r |= w % 64 != 0 and x >= w - w % 64
            ragged_b |= h % 64 != 0 and y >= h - h % 64
        edge |= bool((np.isin(cus["type"], (IC.CU_INTER, IC.CU_INTRA)) & (cus["depth"] <= 3) & ~kept).any())
    for ok, what in ((nxn, "an NxN CU with four different luma modes and its chroma TUs"), (ragged_r, "a TU in the ragged right LCU"),
                     (ragged_b, "a TU in the ragged bottom LCU"), (edge, "a CU record that would leave the picture"),
                     (bad_l, "a luma mode above 34"), (bad_c, "a chroma mode above 34")):
        if not ok:
            missing.append(what)
    # the boundary filter: a luma TU in mode 10 or 26, narrower than 32, predicted differently under implicit_rdpcm
    filt = False
    for case, by, _ in runs:
        if 0 in by and 1 in by:
            filt |= any(a["plane"] == 0 and a["mode"] in (HOR, VER) and a["n"] < 32 and a["pred"] != b["pred"]
                        for a, b in zip(by[0][1]["tus"], by[1][1]["tus"]))
    if not filt:
        missing.append("a luma TU whose prediction differs between implicit_rdpcm 0 and 1")
    tile = False
    for case, by, flat in runs:
        for r, whole in flat.items():
            if whole is not None:
                at = {(t["plane"], t["x"], t["y"]): t["pred"] for t in whole["tus"]}
                tile |= any(at[(t["plane"], t["x"], t["y"])] != t["pred"] for t in by[r][1]["tus"])
    if not tile:
        missing.append("a TU whose prediction differs from the untiled one")
    return missing


def _bytes(a):
    return a.view(np.uint8).reshape(a.shape + (20,))


def store(d, tag, out, chroma):
    for k, n in enumerate("yuv"):
        if k == 0 or chroma:
            d["%s_rec_%s" % (tag, n)], d["%s_coeff_%s" % (tag, n)] = out["rec"][k], out["coeff"][k]
    d[tag + "_cus"], d[tag + "_cbf_out"] = _bytes(out["cus"]), out["cbf_out"]
    d[tag + "_costs"] = out["costs"].view(np.uint32).reshape(out["cus"].shape + (6,))


def build_fixture(B=None, pictures=FIXTURE_PICTURES):
    """numeric arrays only -> (dict, missing coverage).  Per picture the inputs, "<name>_mid_*" = the inter entry over poisoned outputs,
    "<name>_full<r>_*" = the intra entry after it with implicit_rdpcm r"""
    B = B or backend()
    d, runs = {}, []
    for pic in pictures:
        case = fixture_case(pic)
        name, chroma = case["name"], case["chroma"]
        for k, n in enumerate("yuv"):
            if k == 0 or chroma:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = case["src"][k], case["pred"][k]
        d[name + "_cus"], d[name + "_modes"] = _bytes(case["cus"]), case["modes"]
        by, flat = {}, {}
        for r in case["rdpcm"] or (0,):
            by[r] = compose(case, r, B)
            flat[r] = compose(case, r, B, grid=None)[1] if case["grid"] else None
            if r in case["rdpcm"]:
                store(d, "%s_full%d" % (name, r), by[r][1], chroma)
        store(d, name + "_mid", by[sorted(by)[0]][0], chroma)
        runs.append((case, by, flat))
    return d, coverage(runs)


def load_case(z, pic):
    name, w, h, chroma, seed, share, grid, rdpcm = pic
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    return {"name": name, "width": w, "height": h, "chroma": chroma, "grid": grid, "rdpcm": rdpcm, "src": planes("src"), "pred": planes("pred"),
            "cus": np.ascontiguousarray(z[name + "_cus"]).view(CU_INFO).reshape(h // 4, w // 4), "modes": z[name + "_modes"]}


def load_want(z, name, stage, chroma):
    tag = "%s_%s" % (name, stage)
    planes = lambda kind: tuple(z["%s_%s_%s" % (tag, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    costs = np.ascontiguousarray(z[tag + "_costs"])
    cus = np.ascontiguousarray(z[tag + "_cus"])
    return {"rec": planes("rec"), "coeff": planes("coeff"), "cus": cus.view(CU_INFO).reshape(cus.shape[:2]), "cbf_out": z[tag + "_cbf_out"],
            "costs": costs.view(COST).reshape(costs.shape[:2])}


assert_outputs_equal = RC.assert_outputs_equal

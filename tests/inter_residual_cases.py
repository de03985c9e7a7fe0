"""Test-side reference of kvz_hip_inter_residual_frame: a Python walk of the transform tree of kvz_quantize_lcu_residual
(transform.c:424-482) over a CU map, which composes the expected reconstruction, coefficients, flags and cost inputs TU by TU
from the reference's own kvz_quantize_residual, kvz_pixels_calc_ssd and kvz_coeff_abs_sum -- the compiled reference (ref_lib) where
it was built, else the C restatement that the oracle tests pin to it (oracle_lib).  kvz_quantize_lcu_residual itself has no harness
entry, so the tree walk below restates it.  TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import oracle_lib as O
import ref_lib as R
from patterns import CU_INFO

COST = np.dtype([("ssd_y", "<u4"), ("ssd_c", "<u4"), ("zero_ssd_y", "<u4"), ("zero_ssd_c", "<u4"), ("coeff_abs_y", "<u4"), ("coeff_abs_c", "<u4")])
POISON_PIXEL, POISON_COEFF, POISON_CBF, POISON_COST = 0x5A, 0x5A5A, 0xA5, 0x5A5A5A5A


def backend():
    return R if R.available() else O


def xy_to_zorder(width, x, y):
    """cu.h:373-410"""
    assert width in (32, 64) and x % 4 == 0 and y % 4 == 0 and x < width and y < width
    r = 0
    for s in (32, 16, 8, 4):
        if s < width:
            r += (x // s) * s * s + (y // s) * 2 * s * s
            x, y = x % s, y % s
    return r


def inter_cus(cus, width, height):
    """(x, y, size) of every inter CU: a record of type CU_INTER is a CU 64 >> depth wide at its position rounded down to that size;
    one that would leave the picture is skipped (the rule of kvz_hip_inter_recon_frame)"""
    seen = np.zeros(cus.shape, dtype=bool)
    typ, dep = cus["type"].astype(int), cus["depth"].astype(int)
    out = []
    for sy, sx in zip(*np.nonzero(typ == IC.CU_INTER)):
        if seen[sy, sx] or dep[sy, sx] > 3:
            continue
        size = 64 >> dep[sy, sx]
        x, y = (4 * sx) & ~(size - 1), (4 * sy) & ~(size - 1)
        seen[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = True
        if x + size <= width and y + size <= height:
            out.append((int(x), int(y), int(size)))
    return out


def walk_tus(cus, width, height, chroma=1):
    """-> [(plane, x, y, n, cu_x, cu_y)]: the leaf TUs of every inter CU, plane 0 / 1 / 2, (x, y) in LUMA pixels, n the transform
    width.  kvz_quantize_lcu_residual (transform.c:448-481) splits while depth == 0 or tr_depth > depth, reading tr_depth from the
    record at the node's own position; a 4x4 node is a leaf.  Chroma TUs are half as wide, and with 4x4 luma TUs the chroma of an 8x8
    area is one 4x4 TU done at its top-left 4x4 (quantize_tr_residual, transform.c:293-313)."""
    trd = cus["tr_depth"].astype(int)
    out = []

    def node(x, y, depth, cu):
        size = 64 >> depth
        if depth < 4 and (depth == 0 or trd[y // 4, x // 4] > depth):
            for dy in (0, size // 2):
                for dx in (0, size // 2):
                    node(x + dx, y + dy, depth + 1, cu)
            return
        out.append((0, x, y, size) + cu)
        if chroma and (size > 4 or (x % 8 == 0 and y % 8 == 0)):
            for p in (1, 2):
                out.append((p, x, y, max(size // 2, 4)) + cu)
    for (x, y, size) in inter_cus(cus, width, height):
        node(x, y, {64: 0, 32: 1, 16: 2, 8: 3}[size], (x, y))
    return out


def _blocks(plane, xs, ys, n):
    r = ys[:, None] + np.arange(n)
    c = xs[:, None] + np.arange(n)
    return plane[r[:, :, None], c[:, None, :]], (r[:, :, None], c[:, None, :])


def initial_outputs(width, height, chroma=1):
    """poisoned coefficient, cbf_out and cost arrays"""
    n = ((width + 63) // 64) * ((height + 63) // 64)
    coeff = tuple(np.full((n, 1024 if k else 4096), POISON_COEFF, np.int16) if (k == 0 or chroma) else None for k in range(3))
    cost = np.zeros((height // 4, width // 4), COST)
    cost.view(np.uint32)[:] = POISON_COST
    return coeff, np.full((height // 4, width // 4), POISON_CBF, np.uint8), cost


def compose(src, pred, cus, qp, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None, many=False, quantize=None):
    """the outputs of the entry: {"rec", "coeff", "cus", "cbf_out", "costs", "tus": [(plane, n, has)]}.  src, pred: (y, u, v) planes
    (pred may be wider than the picture); init = initial_outputs(...) (default zeros).  many: quantise through
    oracle_lib.quantize_residual_many (host threads) and take the sums with numpy -- for whole frames.  quantize: a stand-in
    quantize(ref, pred, n, plane) -> (rec, coeff, has, ssd, coeff_abs) for the TUs of one size and plane, gathered contiguously."""
    B = B or backend()
    height, width = src[0].shape
    rec = [None if p is None or (k and not chroma) else np.array(p, dtype=np.uint8) for k, p in enumerate(pred)]
    if init is None:
        n = ((width + 63) // 64) * ((height + 63) // 64)
        init = (tuple(np.zeros((n, 1024 if k else 4096), np.int16) if (k == 0 or chroma) else None for k in range(3)),
                np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, COST))
    coeff = [None if c is None else np.array(c) for c in init[0]]
    cbf_out, costs, cus = np.array(init[1]), np.array(init[2]), np.array(cus)
    lcus_x = (width + 63) // 64
    for (x, y, size) in inter_cus(cus, width, height):               # the outputs that TUs accumulate into start from zero
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    tus = walk_tus(cus, width, height, chroma)
    groups = {}
    for t in tus:
        groups.setdefault((t[0], t[3]), []).append(t)
    summary = []
    for (p, n), lst in sorted(groups.items()):
        a = np.array(lst, dtype=np.int64)
        sh = 1 if p else 0
        xs, ys = a[:, 1] >> sh, a[:, 2] >> sh
        ref_b, _ = _blocks(src[p], xs, ys, n)
        pred_b, where = _blocks(rec[p], xs, ys, n)
        own = None
        if quantize:
            r, c, has, *own = quantize(ref_b, pred_b, n, p)
        elif many:
            r, c, has = O.quantize_residual_many(ref_b, pred_b, n, qp, p, 0, 0, slice_is_intra, signhide)
        else:
            r, c, has = B.quantize_residual_batch(ref_b, pred_b, n, qp, p, 0, 0, slice_is_intra, signhide)
        r = r.reshape(-1, n, n)
        rec[p][where] = r
        lx, ly = (a[:, 1] & 63) >> sh, (a[:, 2] & 63) >> sh
        z = np.array([xy_to_zorder(32 if p else 64, int(u), int(v)) for u, v in zip(lx, ly)], dtype=np.int64)
        lcu = (a[:, 2] >> 6) * lcus_x + (a[:, 1] >> 6)
        coeff[p].reshape(-1)[(lcu * (1024 if p else 4096) + z)[:, None] + np.arange(n * n)] = c.reshape(-1, n * n)
        span = (2 * n if p else n) // 4                               # SCUs the TU covers, per axis
        sr = (a[:, 2] >> 2)[:, None] + np.arange(span)
        sc = (a[:, 1] >> 2)[:, None] + np.arange(span)
        scu = (sr[:, :, None], sc[:, None, :])
        flag = (has != 0).astype(np.uint8)[:, None, None]
        if p == 0:
            cus["cbf_y"][scu] = flag                                  # lcu_set_coeff (search.c:173-190)
        cbf_out[scu] |= (flag << p)
        if many or own:
            d = ref_b.astype(np.int64) - r
            dz = ref_b.astype(np.int64) - pred_b
            ssd, zssd = (d * d).sum(axis=(1, 2)), (dz * dz).sum(axis=(1, 2))
            sab = np.abs(c.astype(np.int64)).reshape(len(lst), -1).sum(axis=1)
        else:
            ssd = np.array([B.pixels_calc_ssd(ref_b[i], 0, r[i], 0, n, n, n) for i in range(len(lst))], dtype=np.int64)
            zssd = np.array([B.pixels_calc_ssd(ref_b[i], 0, pred_b[i], 0, n, n, n) for i in range(len(lst))], dtype=np.int64)
            sab = np.array([B.coeff_abs_sum(c[i]) for i in range(len(lst))], dtype=np.int64)
        if own:
            ssd, sab = own[0].astype(np.int64), own[1].astype(np.int64)
        at = (a[:, 5] >> 2, a[:, 4] >> 2)
        for name, v in (("ssd", ssd), ("zero_ssd", zssd), ("coeff_abs", sab)):
            f = costs[name + ("_c" if p else "_y")]
            np.add.at(f, at, v.astype(np.uint32))
        summary += [(p, n, int(h)) for h in has]
    return {"rec": tuple(rec), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": summary}


def make_map(w, h, seed, deep_share=0.2, edge_cu=True, **kw):
    """IC.random_cu_map with tr_depth filled in as search.c:572-576 sets it for an inter CU -- max(1, depth), depth + 1 for a part mode
    other than 2Nx2N -- and a share of CUs one or two levels deeper (the entry must read tr_depth from the map).  edge_cu: an inter
    record of a 32x32 CU in a ragged last LCU row, which leaves the picture and must be skipped."""
    cus, ref_LX = IC.random_cu_map(w, h, seed, **kw)
    g = np.random.default_rng(seed + 7)
    if edge_cu and h % 32:
        blk = cus[(h - h % 32) // 4:, 0:8]
        blk["type"], blk["depth"], blk["part_size"], blk["mv_dir"], blk["mv_ref"] = IC.CU_INTER, 1, 0, 1, 0
    for (x, y, size) in inter_cus(cus, w, h):
        depth = {64: 0, 32: 1, 16: 2, 8: 3}[size]
        trd = max(1, depth) if cus[y // 4, x // 4]["part_size"] == 0 else depth + 1
        if g.random() < deep_share:
            trd = min(4, trd + int(g.integers(1, 3)))
        cus[y // 4:(y + size) // 4, x // 4:(x + size) // 4]["tr_depth"] = trd
    return cus, ref_LX


def make_source(pred, cus, seed, chroma=1, amps=(0, 0, 0, 1, 2, 3, 5, 8, 14, 24, 48)):
    """source planes = prediction + noise of one amplitude per CU (0 among them: TUs without coefficients), of the picture size
    cus.shape * 4"""
    g = np.random.default_rng(seed)
    hs, ws = cus.shape
    h, w = 4 * hs, 4 * ws
    amp = np.zeros(cus.shape, dtype=np.int64)
    for (x, y, size) in inter_cus(cus, w, h):
        amp[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = amps[int(g.integers(0, len(amps)))]
    out = []
    for k in range(3 if chroma else 1):
        a = np.kron(amp, np.ones((2, 2) if k else (4, 4), dtype=np.int64))
        ph, pw = a.shape
        noise = np.rint((g.random((ph, pw)) * 2 - 1) * a).astype(np.int64)
        out.append(np.clip(pred[k][:ph, :pw].astype(np.int64) + noise, 0, 255).astype(np.uint8))
    return tuple(out) if chroma else (out[0], None, None)


def smooth_planes(w, h, seed, chroma=1, pad=0):
    """a stand-in prediction: low-contrast texture over the full range, `pad` extra poisoned columns (a stride beyond the width)"""
    g = np.random.default_rng(seed)
    out = []
    for k in range(3 if chroma else 1):
        pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
        yy, xx = np.mgrid[0:ph, 0:pw]
        img = (xx * 3 + yy * 5) % 256 + g.integers(-6, 7, (ph, pw))
        a = np.full((ph, pw + pad), POISON_PIXEL, np.uint8)
        a[:, :pw] = np.clip(img, 0, 255)
        out.append(a)
    return tuple(out) if chroma else (out[0], None, None)


# the pictures of tests/golden/inter_residual.npz: (name, width, height, chroma, qp, signhide, seed)
FIXTURE_PICTURES = (("ragged", 200, 136, 1, 22, 0, 51), ("mono", 96, 72, 0, 32, 0, 52), ("hide", 128, 128, 1, 37, 1, 53))


def fixture_case(name, w, h, chroma, qp, signhide, seed):
    cus, _ = make_map(w, h, seed, intra_share=0.12, blank_share=0.08)
    pred = smooth_planes(w, h, seed + 100, chroma)
    return make_source(pred, cus, seed + 200, chroma), pred, cus


def coverage(tus, cus_by_picture):
    """the condition the fixture must meet: both flag values for every luma and chroma TU size; a 64x64 CU, an 8x8 CU with 4x4 luma TUs,
    intra and blank records and a CU skipped at the ragged edge.  -> list of what is missing"""
    missing = []
    for (p, sizes) in ((0, (4, 8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
        for n in sizes:
            for has in (0, 1):
                if not any(t[0] == p and t[1] == n and t[2] == has for t in tus):
                    missing.append("plane %d size %d has_coeffs %d" % (p, n, has))
    has64 = has8x4 = intra = blank = edge = False
    for (cus, w, h) in cus_by_picture:
        kept = inter_cus(cus, w, h)
        has64 |= any(s == 64 for (_, _, s) in kept)
        has8x4 |= any(s == 8 and cus[y // 4, x // 4]["tr_depth"] == 4 for (x, y, s) in kept)
        intra |= bool((cus["type"] == IC.CU_INTRA).any())
        blank |= bool((cus["type"] == 0).any())
        m = np.zeros(cus.shape, bool)
        for (x, y, s) in kept:
            m[y // 4:(y + s) // 4, x // 4:(x + s) // 4] = True
        edge |= bool(((cus["type"] == IC.CU_INTER) & (cus["depth"] <= 3) & ~m).any())
    for ok, what in ((has64, "a 64x64 CU"), (has8x4, "an 8x8 CU with 4x4 TUs"), (intra, "intra records"), (blank, "blank records"), (edge, "an edge-skipped CU")):
        if not ok:
            missing.append(what)
    return missing


def build_fixture(B=None):
    """numeric arrays only: per picture the source and prediction planes, the CU map (as bytes) and, over poisoned outputs, the expected
    planes, coefficients, CU map, cbf_out and costs (as uint32 [.., 6]).  -> (dict, missing coverage)"""
    d, tus, maps = {}, [], []
    for (name, w, h, chroma, qp, signhide, seed) in FIXTURE_PICTURES:
        src, pred, cus = fixture_case(name, w, h, chroma, qp, signhide, seed)
        want = compose(src, pred, cus, qp, chroma, signhide, B=B, init=initial_outputs(w, h, chroma))
        tus += want["tus"]
        maps.append((cus, w, h))
        for k, n in enumerate("yuv"):
            if src[k] is not None:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = src[k], pred[k]
                d["%s_rec_%s" % (name, n)], d["%s_coeff_%s" % (name, n)] = want["rec"][k], want["coeff"][k]
        d[name + "_cus"] = cus.view(np.uint8).reshape(cus.shape + (20,))
        d[name + "_cus_out"] = want["cus"].view(np.uint8).reshape(cus.shape + (20,))
        d[name + "_cbf_out"] = want["cbf_out"]
        d[name + "_costs"] = want["costs"].view(np.uint32).reshape(cus.shape + (6,))
        d[name + "_tus"] = np.array(want["tus"], dtype=np.int32).reshape(-1, 3)
    return d, coverage(tus, maps)


def load_fixture_case(z, name, chroma):
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    view = lambda a: np.ascontiguousarray(a).view(CU_INFO).reshape(a.shape[:2])
    want = {"rec": planes("rec"), "coeff": planes("coeff"), "cus": view(z[name + "_cus_out"]), "cbf_out": z[name + "_cbf_out"],
            "costs": np.ascontiguousarray(z[name + "_costs"]).view(COST).reshape(z[name + "_costs"].shape[:2])}
    return planes("src"), planes("pred"), view(z[name + "_cus"]), want


def assert_outputs_equal(got, want, what="", chroma=1):
    for k, n in enumerate("yuv"):
        if k and not chroma:
            continue
        np.testing.assert_array_equal(got["rec"][k], want["rec"][k], err_msg="%s rec %s" % (what, n))
        np.testing.assert_array_equal(got["coeff"][k], want["coeff"][k], err_msg="%s coeff %s" % (what, n))
    np.testing.assert_array_equal(got["cus"].view(np.uint8), want["cus"].view(np.uint8), err_msg=what + " cus")
    np.testing.assert_array_equal(got["cbf_out"], want["cbf_out"], err_msg=what + " cbf_out")
    np.testing.assert_array_equal(got["costs"].view(np.uint32), want["costs"].view(np.uint32), err_msg=what + " costs")

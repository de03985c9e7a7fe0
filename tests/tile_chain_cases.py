"""Test-side reference of the four tile entries of the picture chain: kvz_hip_intra_recon_frame_tiles, kvz_hip_cu_qp_frame_tiles,
kvz_hip_deblock_frame_tiles and kvz_hip_sao_frame_tiles.

The reference runs everything in-loop on state->tile->frame, a sub-picture with its own origin and size.  So the expected values are
the existing compositions of the reference's own functions (lcu_qp_cases.compose_intra and set_cu_qps, the backend's deblock_frame,
sao_frame_cases.compose_recon) run on every tile as a picture of its own -- contiguous crops of the planes, the CU map, the modes, the
cbf bytes and the tile's per-LCU values -- and stitched back; tile-local LCU arrays map to picture raster order.  The backend is the
compiled reference (ref_lib) where it was built, else the oracle (oracle_lib).  TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import ref_lib as R
import sao_frame_cases as SC
from patterns import CU_INFO, deblock_params

COST = RC.COST


def backend():
    return R if R.available() else O


# ---------------------------------------------------------------- grids
def uniform_bd(n, c):
    """the reference's uniform spacing (encoder.c:437-458)"""
    bd = [0]
    for i in range(c):
        bd.append(bd[-1] + (i + 1) * n // c - i * n // c)
    return bd


def one_tile(width, height):
    lx, ly = QC.lcu_grid(width, height)
    return [0, lx], [0, ly]


def tiles(width, height, col_bd, row_bd):
    """[(x0, y0, x1, y1, lcus)] in luma pixels, in the tiles' raster order; lcus: the picture raster indices of the tile's LCUs in the
    tile's own raster order"""
    lx, ly = QC.lcu_grid(width, height)
    assert col_bd[0] == 0 and row_bd[0] == 0 and col_bd[-1] == lx and row_bd[-1] == ly
    out = []
    for j in range(len(row_bd) - 1):
        for i in range(len(col_bd) - 1):
            lcus = [r * lx + c for r in range(row_bd[j], row_bd[j + 1]) for c in range(col_bd[i], col_bd[i + 1])]
            out.append((64 * col_bd[i], 64 * row_bd[j], min(64 * col_bd[i + 1], width), min(64 * row_bd[j + 1], height), np.array(lcus)))
    return out


def crop_planes(planes, t, n_planes):
    x0, y0, x1, y1 = t[:4]
    return tuple(np.ascontiguousarray(p[(y0 >> (k > 0)):(y1 >> (k > 0)), (x0 >> (k > 0)):(x1 >> (k > 0))]) if k < n_planes else None
                 for k, p in enumerate(planes))


def crop_map(a, t):
    x0, y0, x1, y1 = t[:4]
    return np.ascontiguousarray(a[y0 // 4:y1 // 4, x0 // 4:x1 // 4])


def paste_planes(dst, part, t, n_planes):
    x0, y0, x1, y1 = t[:4]
    for k in range(n_planes):
        s = 1 if k else 0
        dst[k][y0 >> s:y1 >> s, x0 >> s:x1 >> s] = part[k][:(y1 - y0) >> s, :(x1 - x0) >> s]


# ---------------------------------------------------------------- the four stages, tile by tile
def compose_intra(src, rec, cus, modes, lcu_qp, col_bd, row_bd, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None):
    """kvz_hip_intra_recon_frame_tiles as QC.compose_intra returns it; "tus" carry picture coordinates"""
    height, width = src[0].shape
    n = 3 if chroma else 1
    if init is None:
        init = QC.zero_outputs(width, height, chroma)
        init = (tuple(np.zeros_like(c) if c is not None else None for c in init[0]), init[1], np.zeros(cus.shape, COST))
    out = {"rec": [np.array(p[:height >> (k > 0), :width >> (k > 0)], dtype=np.uint8) for k, p in enumerate(rec[:n])],
           "coeff": [np.array(c) for c in init[0][:n]], "cus": np.array(cus), "cbf_out": np.array(init[1]), "costs": np.array(init[2]), "tus": []}
    q = np.asarray(lcu_qp).reshape(-1)
    for t in tiles(width, height, col_bd, row_bd):
        sub_init = (tuple(np.ascontiguousarray(out["coeff"][k][t[4]]) if k < n else None for k in range(3)), crop_map(out["cbf_out"], t),
                    crop_map(out["costs"], t))
        r = QC.compose_intra(crop_planes(src, t, n), crop_planes(out["rec"] + [None] * (3 - n), t, n), crop_map(cus, t), crop_map(modes, t), q[t[4]],
                             chroma, signhide, slice_is_intra, B=B, init=sub_init)
        paste_planes(out["rec"], r["rec"], t, n)
        for k in range(n):
            out["coeff"][k][t[4]] = r["coeff"][k]
        blk = (slice(t[1] // 4, t[3] // 4), slice(t[0] // 4, t[2] // 4))
        out["cus"][blk], out["cbf_out"][blk], out["costs"][blk] = r["cus"], r["cbf_out"], r["costs"]
        out["tus"] += [u[:5] + (u[5] + t[0], u[6] + t[1]) + u[7:] for u in r["tus"]]
    pad = [None] * (3 - n)
    out["rec"], out["coeff"] = tuple(out["rec"] + pad), tuple(out["coeff"] + pad)
    return out


def set_cu_qps(cus, cbf, lcu_qp, start_qp, col_bd, row_bd, chain_rows=0):
    """kvz_hip_cu_qp_frame_tiles -> (records with qp written, lcu_last_qp in picture raster order)"""
    hs, ws = cus.shape
    out, q = np.array(cus), np.asarray(lcu_qp).reshape(-1)
    last = np.zeros(q.size, np.int8)
    for t in tiles(4 * ws, 4 * hs, col_bd, row_bd):
        w_lcus = (t[2] - t[0] + 63) // 64
        c, l = QC.set_cu_qps(crop_map(cus, t), crop_map(np.asarray(cbf), t), q[t[4]], start_qp, w_lcus if chain_rows else 0)
        out[t[1] // 4:t[3] // 4, t[0] // 4:t[2] // 4] = c
        last[t[4]] = l
    return out, last


def deblock(rec, cus, prm, col_bd, row_bd, B=None):
    """kvz_hip_deblock_frame_tiles -> (y, u, v)"""
    B = B or backend()
    height, width = rec[0].shape
    n = 3 if int(np.asarray(prm)["chroma"][0]) else 1
    out = [np.array(p, dtype=np.uint8) for p in rec[:n]]
    for t in tiles(width, height, col_bd, row_bd):
        p = crop_planes(rec, t, n)
        paste_planes(out, B.deblock_frame(p[0], p[1], p[2], crop_map(cus, t), prm), t, n)
    return tuple(out + [None] * (3 - n))


def sao(rec, sao_luma, sao_chroma, col_bd, row_bd, chroma=1, B=None):
    """kvz_hip_sao_frame_tiles -> (y, u, v)"""
    height, width = rec[0].shape
    n = 3 if chroma else 1
    out = [np.array(p, dtype=np.uint8) for p in rec[:n]]
    for t in tiles(width, height, col_bd, row_bd):
        part = SC.compose_recon(crop_planes(rec, t, n), np.asarray(sao_luma)[t[4]], np.asarray(sao_chroma)[t[4]] if chroma else None, chroma, B)
        paste_planes(out, part, t, n)
    return tuple(out + [None] * (3 - n))


def sao_stats(src, rec, col_bd, row_bd, chroma=1, B=None):
    """kvz_hip_sao_stats_frame composed tile by tile (the entry does not depend on tiles: this must equal SC.compose_stats)"""
    height, width = src[0].shape
    n = 3 if chroma else 1
    out = np.zeros((n, QC.lcu_grid(width, height)[0] * QC.lcu_grid(width, height)[1]), dtype=SC.STATS)
    for t in tiles(width, height, col_bd, row_bd):
        out[:, t[4]] = SC.compose_stats(crop_planes(src, t, n), crop_planes(rec, t, n), chroma, B)
    return out


def inter_residual(src, pred, cus, qp, col_bd, row_bd, chroma=1, signhide=0, B=None, init=None):
    """kvz_hip_inter_residual_frame composed tile by tile (again: must equal RC.compose)"""
    height, width = src[0].shape
    n = 3 if chroma else 1
    init = init or RC.initial_outputs(width, height, chroma)
    out = {"rec": [np.array(p[:height >> (k > 0), :width >> (k > 0)], dtype=np.uint8) for k, p in enumerate(pred[:n])],
           "coeff": [np.array(c) for c in init[0][:n]], "cus": np.array(cus), "cbf_out": np.array(init[1]), "costs": np.array(init[2])}
    for t in tiles(width, height, col_bd, row_bd):
        sub_init = (tuple(np.ascontiguousarray(out["coeff"][k][t[4]]) if k < n else None for k in range(3)), crop_map(out["cbf_out"], t),
                    crop_map(out["costs"], t))
        r = RC.compose(crop_planes(src, t, n), crop_planes(out["rec"] + [None] * (3 - n), t, n), crop_map(cus, t), qp, chroma, signhide, B=B, init=sub_init)
        paste_planes(out["rec"], r["rec"], t, n)
        for k in range(n):
            out["coeff"][k][t[4]] = r["coeff"][k]
        blk = (slice(t[1] // 4, t[3] // 4), slice(t[0] // 4, t[2] // 4))
        out["cus"][blk], out["cbf_out"][blk], out["costs"][blk] = r["cus"], r["cbf_out"], r["costs"]
    pad = [None] * (3 - n)
    out["rec"], out["coeff"] = tuple(out["rec"] + pad), tuple(out["coeff"] + pad)
    return out


def compose_chain(case, B=None, grid=None):
    """inter residual (no tiles in it) -> intra -> QP map (both chain_rows) -> deblocking with per_cu_qp = 1 on the chain_rows 0 map -> SAO.
    grid: (col_bd, row_bd), default the case's; one_tile(...) gives the untiled chain.  -> dict of the stages' outputs"""
    w, h, chroma = case["width"], case["height"], case["chroma"]
    col_bd, row_bd = grid or (case["col_bd"], case["row_bd"])
    init = QC.zero_outputs(w, h, chroma)
    mid = QC.compose_inter(case["src"], case["pred"], case["cus"], case["lcu_qp"], chroma, case["signhide"], case["slice_is_intra"], B=B, init=init)
    full = compose_intra(case["src"], mid["rec"], mid["cus"], case["modes"], case["lcu_qp"], col_bd, row_bd, chroma, case["signhide"],
                         case["slice_is_intra"], B=B, init=(mid["coeff"], mid["cbf_out"], mid["costs"]))
    mapped, last = set_cu_qps(full["cus"], full["cbf_out"], case["lcu_qp"], case["start_qp"], col_bd, row_bd, 0)
    rows, last_rows = set_cu_qps(full["cus"], full["cbf_out"], case["lcu_qp"], case["start_qp"], col_bd, row_bd, 1)
    deb = deblock(full["rec"], mapped, chain_deblock_params(case), col_bd, row_bd, B)
    dst = sao(deb, case["sao_luma"], case["sao_chroma"], col_bd, row_bd, chroma, B)
    return {"mid": mid, "full": full, "cus_qp": mapped, "last": last, "cus_qp_rows": rows, "last_rows": last_rows, "deb": deb, "sao": dst}


def chain_deblock_params(case):
    return deblock_params(qp=case["start_qp"], per_cu_qp=1, chroma=case["chroma"])


# ---------------------------------------------------------------- the pictures of tests/golden/tile_chain.npz
# (name, width, height, chroma, signhide, slice_is_intra, seed, intra_share, start_qp, col_bd, row_bd)
FIXTURE_PICTURES = (
    ("ragged", 200, 136, 1, 1, 0, 175, 0.45, 30, (0, 1, 4), (0, 2, 3)),
    ("columns", 192, 64, 1, 0, 1, 172, 1.0, 33, (0, 1, 2, 3), (0, 1)),
    ("mono", 96, 72, 0, 0, 0, 173, 0.45, 27, (0, 1, 2), (0, 1, 2)),
)
QUIET = {"ragged": ((64, 0), (0, 64), (64, 64), (0, 128)), "mono": ((64, 0), (0, 64))}     # LCUs whose first CU is made an uncoded inter CU

STEEP = {"ragged": ((32, 64, 64),)}          # (x0, y, x1): the intra CUs that begin in this run of an LCU's top row get mode 34, luma and chroma


def quiet_first_cu(src, pred, cus, modes, x, y, chroma):
    """the first CU of the LCU at (x, y) becomes an inter CU whose source is its prediction: no coefficients, so set_cu_qps gives it
    the predictor"""
    size = 64 >> min(int(cus["depth"][y // 4, x // 4]), 3)
    blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
    cus["type"][blk], cus["mv_dir"][blk], cus["part_size"][blk] = IC.CU_INTER, 1, 0
    modes[blk] = XC.POISON_MODE
    for k in range(3 if chroma else 1):
        s = 1 if k else 0
        src[k][y >> s:(y + size) >> s, x >> s:(x + size) >> s] = pred[k][y >> s:(y + size) >> s, x >> s:(x + size) >> s]


def sao_records(w, h, seed, col_bd, row_bd):
    """int32 [LCUs, 14] for luma and chroma: edge records whose class walks with lx + ly, so that all four classes stand on both sides of
    every boundary; every seventh LCU a band record, every eleventh a copy"""
    g = np.random.default_rng(seed)
    lx, ly = QC.lcu_grid(w, h)
    out = []
    for shift in (0, 1):
        s = np.zeros((lx * ly, 14), np.int32)
        for j in range(ly):
            for i in range(lx):
                r, n = s[j * lx + i], j * lx + i
                r[0] = 1 if n % 7 == 3 else (0 if n % 11 == 7 else 2)
                r[1] = (i + j + shift) % 4
                r[2:4] = g.integers(0, 29, 2)
                r[4:9], r[9:14] = (0, 3, 1, -1, -3), (0, 2, 1, -2, -4)
        out.append(s)
    return out[0], out[1]


def fixture_case(name, w, h, chroma, signhide, slice_is_intra, seed, intra_share, start_qp, col_bd, row_bd):
    """-> dict: the inputs of the chain.  Every record is an inter CU with motion or an intra CU (the reference's deblocking filter takes
    no blank record, lcu_qp_cases.chain_case); the source is the prediction plus noise inside the inter CUs and a picture of its own
    inside the intra CUs; a QP per LCU from 22..42"""
    cus, _, modes = XC.make_map(w, h, seed, intra_share=intra_share, blank_share=0.0, bad_share=0.0, edge_cu=False)
    pred = RC.smooth_planes(w, h, seed + 1, chroma)
    inter_src = RC.make_source(pred, cus, seed + 2, chroma)
    intra_src, _ = XC.make_planes(cus, seed + 3, chroma)
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = [np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) if (k == 0 or chroma) else None for k in range(3)]
    for (x, y) in QUIET.get(name, ()):
        quiet_first_cu(src, pred, cus, modes, x, y, chroma)
    for (x0, y, x1) in STEEP.get(name, ()):
        for (x, yy, size) in XC.intra_cus(cus, w, h):
            if yy == y and x0 <= x < x1:
                modes[yy // 4:(yy + size) // 4, x // 4:(x + size) // 4] = 34       # the above-right run ends at the tile's edge
    lx, ly = QC.lcu_grid(w, h)
    lcu_qp = np.random.default_rng(seed + 4).integers(22, 43, lx * ly).astype(np.int8)
    luma, chro = sao_records(w, h, seed + 5, col_bd, row_bd)
    return {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": slice_is_intra, "start_qp": start_qp,
            "col_bd": list(col_bd), "row_bd": list(row_bd), "src": tuple(src), "pred": pred, "cus": cus, "modes": modes, "lcu_qp": lcu_qp,
            "sao_luma": luma, "sao_chroma": chro if chroma else None}


# ---------------------------------------------------------------- what the fixture must contain
def _near(shape, sh, col_bd, row_bd, reach):
    """masks of the pixels of a plane within `reach` of an inner vertical / horizontal tile boundary"""
    ph, pw = shape
    v, hz = np.zeros(shape, bool), np.zeros(shape, bool)
    for b in col_bd[1:-1]:
        x = (64 * b) >> sh
        v[:, max(0, x - reach):x + reach] = True
    for b in row_bd[1:-1]:
        y = (64 * b) >> sh
        hz[max(0, y - reach):y + reach] = True
    return v, hz


def coverage(cases, tiled, untiled):
    """what the fixture pictures fail to exercise -> list.  cases: the inputs; tiled / untiled: compose_chain of each with its grid and
    with one tile"""
    missing = []
    left, top, right, sizes = set(), set(), set(), set()
    intra_v = intra_h = False
    deb = {(k, p): False for k in "vh" for p in ("luma", "chroma")}
    classes = {"v": set(), "h": set()}
    sao_diff = set()
    restart = rows_differ = False
    for case, t, u in zip(cases, tiled, untiled):
        col_bd, row_bd, chroma = case["col_bd"], case["row_bd"], case["chroma"]
        xs, ys = [64 * b for b in col_bd[1:-1]], [64 * b for b in row_bd[1:-1]]
        for (p, n, has, mode, scan, x, y, leaf, sh_, qp) in t["full"]["tus"]:
            ext = n * (2 if p else 1)
            sizes.add(n if p == 0 else None)
            if x in xs and mode <= 10:
                left.add(p > 0)
            if y in ys and (mode <= 1 or mode >= 26):
                top.add(p > 0)
            tile_top = max(b for b in [64 * r for r in row_bd] if b <= y)
            if x + ext in xs and mode > 26 and y % 64 == 0 and y > tile_top:
                right.add(p > 0)
        n_planes = 3 if chroma else 1
        # what the untiled stages do to the tiled chain's own planes
        whole_deb = backend().deblock_frame(t["full"]["rec"][0], t["full"]["rec"][1], t["full"]["rec"][2], t["cus_qp"], chain_deblock_params(case))
        whole_sao = SC.compose_recon(t["deb"], case["sao_luma"], case["sao_chroma"], chroma)
        for k in range(n_planes):
            sh = 1 if k else 0
            v, hz = _near(t["full"]["rec"][k].shape, sh, col_bd, row_bd, 1)
            d = t["full"]["rec"][k] != u["full"]["rec"][k]
            intra_v |= bool((d & v).any())
            intra_h |= bool((d & hz).any())
            # deblocking: a pixel at the boundary that the untiled filter modifies and the tiled one leaves as it was
            whole = whole_deb
            for key, m in (("v", v), ("h", hz)):
                hit = (whole[k] != t["full"]["rec"][k]) & (t["deb"][k] == t["full"]["rec"][k]) & m
                deb[(key, "chroma" if k else "luma")] |= bool(hit.any())
            infos = case["sao_luma"] if k == 0 else case["sao_chroma"]
            whole = whole_sao
            lx = QC.lcu_grid(case["width"], case["height"])[0]
            yy, xx = np.mgrid[0:whole[k].shape[0], 0:whole[k].shape[1]]
            lcu = (yy >> (6 - sh)) * lx + (xx >> (6 - sh))
            for i, s in enumerate(infos):
                if s[0] != 2:
                    continue
                mine = lcu == i
                if (mine & v).any():
                    classes["v"].add(int(s[1]))
                if (mine & hz).any():
                    classes["h"].add(int(s[1]))
                if ((whole[k] != t["sao"][k]) & mine & (v | hz)).any():
                    sao_diff.add(int(s[1]))
        first = [(64 * c, 64 * r) for r in row_bd[:-1] for c in col_bd[:-1]][1:]
        restart |= any(t["cus_qp"]["qp"][y // 4, x // 4] == case["start_qp"] != u["cus_qp"]["qp"][y // 4, x // 4] for (x, y) in first)
        rows_differ |= not np.array_equal(t["cus_qp"]["qp"], t["cus_qp_rows"]["qp"])
    for name, got in (("at the left edge of a tile column whose mode reads the left references", left),
                      ("at the top edge of a tile row whose mode reads the top references", top),
                      ("at the right edge of a tile column with a mode above 26 and an above-right run that the tile cuts", right)):
        for chroma_tu in (False, True):
            if chroma_tu not in got:
                missing.append("intra: a %s TU %s" % ("chroma" if chroma_tu else "luma", name))
    missing += ["intra: a luma TU %d wide" % n for n in (4, 8, 16, 32) if n not in sizes]
    if not intra_v:
        missing.append("intra: tiled != untiled next to a vertical boundary")
    if not intra_h:
        missing.append("intra: tiled != untiled next to a horizontal boundary")
    missing += ["deblocking: a %s edge on a %s boundary that only the untiled filter modifies" % (p, {"v": "vertical", "h": "horizontal"}[k])
                for (k, p), ok in deb.items() if not ok]
    for key, what in (("v", "vertical"), ("h", "horizontal")):
        missing += ["SAO: an edge record of class %d in an LCU at a %s boundary" % (c, what) for c in range(4) if c not in classes[key]]
    missing += ["SAO: a boundary pixel of class %d that differs between tiled and untiled" % c for c in range(4) if c not in sao_diff]
    if not restart:
        missing.append("QP map: a tile whose first LCU starts with an uncoded CU and would otherwise inherit another QP")
    if not rows_differ:
        missing.append("QP map: chain_rows 0 and 1 giving different maps")
    return missing


# ---------------------------------------------------------------- the fixture
def _bytes(a):
    return a.view(np.uint8).reshape(a.shape + (20,))


def build_fixture(B=None):
    """numeric arrays only -> (dict, missing coverage)"""
    d, cases, tiled, untiled = {}, [], [], []
    for pic in FIXTURE_PICTURES:
        case = fixture_case(*pic)
        name, chroma = case["name"], case["chroma"]
        t = compose_chain(case, B)
        cases.append(case)
        tiled.append(t)
        untiled.append(compose_chain(case, B, one_tile(case["width"], case["height"])))
        for k, n in enumerate("yuv"):
            if k == 0 or chroma:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = case["src"][k], case["pred"][k]
                d["%s_rec_%s" % (name, n)], d["%s_coeff_%s" % (name, n)] = t["full"]["rec"][k], t["full"]["coeff"][k]
                d["%s_deb_%s" % (name, n)], d["%s_sao_%s" % (name, n)] = t["deb"][k], t["sao"][k]
        d[name + "_cus"], d[name + "_modes"], d[name + "_lcu_qp"] = _bytes(case["cus"]), case["modes"], case["lcu_qp"]
        d[name + "_col_bd"], d[name + "_row_bd"] = np.array(case["col_bd"], np.int32), np.array(case["row_bd"], np.int32)
        d[name + "_sao_luma"] = case["sao_luma"]
        if chroma:
            d[name + "_sao_chroma"] = case["sao_chroma"]
        d[name + "_cus_out"], d[name + "_cbf_out"] = _bytes(t["full"]["cus"]), t["full"]["cbf_out"]
        d[name + "_costs"] = t["full"]["costs"].view(np.uint32).reshape(case["cus"].shape + (6,))
        d[name + "_cus_qp"], d[name + "_cus_qp_rows"] = _bytes(t["cus_qp"]), _bytes(t["cus_qp_rows"])
        d[name + "_last"], d[name + "_last_rows"] = t["last"], t["last_rows"]
    return d, coverage(cases, tiled, untiled)


def load_fixture_case(z, pic):
    """-> (case as fixture_case returns it, want as compose_chain returns it without "mid" and "tus")"""
    name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, col_bd, row_bd = pic
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    view = lambda a: np.ascontiguousarray(a).view(CU_INFO).reshape(a.shape[:2])
    case = {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": slice_is_intra, "start_qp": start_qp,
            "col_bd": z[name + "_col_bd"].tolist(), "row_bd": z[name + "_row_bd"].tolist(), "src": planes("src"), "pred": planes("pred"),
            "cus": view(z[name + "_cus"]), "modes": z[name + "_modes"], "lcu_qp": z[name + "_lcu_qp"], "sao_luma": z[name + "_sao_luma"],
            "sao_chroma": z[name + "_sao_chroma"] if chroma else None}
    costs = np.ascontiguousarray(z[name + "_costs"]).view(COST).reshape(z[name + "_costs"].shape[:2])
    full = {"rec": planes("rec"), "coeff": planes("coeff"), "cus": view(z[name + "_cus_out"]), "cbf_out": z[name + "_cbf_out"], "costs": costs}
    want = {"full": full, "cus_qp": view(z[name + "_cus_qp"]), "cus_qp_rows": view(z[name + "_cus_qp_rows"]), "last": z[name + "_last"],
            "last_rows": z[name + "_last_rows"], "deb": planes("deb"), "sao": planes("sao")}
    return case, want

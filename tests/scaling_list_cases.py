"""Test-side reference of the scaling-list entries of the picture chain: kvz_hip_scaling_tables_pack, kvz_hip_inter_residual_frame_sl and
kvz_hip_intra_recon_frame_sl.

Three parts.  (1) process_lists: a RESTATEMENT of kvz_scalinglist_set / kvz_scalinglist_process (scalinglist.c:277-411), from list
coefficients and DC values to the processed tables, and dense(), the packed layout of kvz_hip_scaling_tables.  (2) Listed: a backend that
forwards everything to ref_lib or oracle_lib except quantize_residual_batch, which picks the TU's tables by the rule of the entries and
calls the oracle with them (or the compiled reference with its default lists): handed as `B` to the existing compositions
(inter_residual_cases, lcu_qp_cases, tile_chain_cases) it gives the expected outputs without a second tree walk.  It also keeps a log
of every TU it quantised, which coverage() reads.  (3) The pictures of tests/golden/scaling_list.npz.  TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import ref_lib as R
import tile_chain_cases as TC
from patterns import CU_INFO, deblock_params

COST = RC.COST
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)            # scalinglist.c:66
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)                          # scalinglist.c:67
LIST_NUM = (6, 6, 6, 2)                                              # kvz_g_scaling_list_num, scalinglist.c:30
TABLE_LEN = 36 * (16 + 64 + 256 + 1024)
CHROMA_SCALE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32,
                33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51)   # transform.c:129-143


def scaled_qp(plane, qp):
    return qp if plane == 0 else CHROMA_SCALE[min(max(qp, 0), 57)]


# ---------------------------------------------------------------- (1) the lists
def process_lists(coeff, dc):
    """kvz_scalinglist_process with enable = 1.  coeff[size_id]: [LIST_NUM[size_id], 16 or 64] list coefficients (scaling_list_coeff);
    dc[size_id][list]: scaling_list_dc, 0 = 16.  -> {(size_id, list, rem): (quant, dequant)} as int32 [N * N]; (3, 3, rem) is the
    alias of (3, 1, rem) (scalinglist.c:91-95), (3, 2 / 4 / 5, rem) do not exist."""
    out = {}
    for size_id in range(4):
        n = 4 << size_id
        size_num = min(8, n)
        ratio = n // size_num
        j, i = np.mgrid[0:n, 0:n]
        pos = (size_num * (j // ratio) + i // ratio).reshape(-1)
        for lst in range(LIST_NUM[size_id]):
            c = np.asarray(coeff[size_id][lst], dtype=np.int64)
            d = int(dc[size_id][lst]) or 16
            for rem in range(6):
                q = (QUANT_SCALES[rem] << 4) // c[pos]                # kvz_scalinglist_process_enc, :321-324
                dq = INV_QUANT_SCALES[rem] * c[pos]                   # scalinglist_process_dec, :291-295
                if ratio > 1:
                    q[0], dq[0] = (QUANT_SCALES[rem] << 4) // d, INV_QUANT_SCALES[rem] * d
                out[(size_id, lst, rem)] = (q.astype(np.int32), dq.astype(np.int32))
    for rem in range(6):
        out[(3, 3, rem)] = out[(3, 1, rem)]
    return out


def table_offset(size_id, lst, rem):
    """the layout of kvz_hip_scaling_tables, from its statement in kvz_hip.h"""
    return 36 * (0, 16, 80, 336)[size_id] + (6 * lst + rem) * (4 << size_id) ** 2


def dense(tables):
    """-> (quant, dequant): the two packed arrays; the three 32x32 lists that do not exist stay zero"""
    q, d = np.zeros(TABLE_LEN, np.int32), np.zeros(TABLE_LEN, np.int32)
    for (size_id, lst, rem), (tq, td) in tables.items():
        at = table_offset(size_id, lst, rem)
        q[at:at + tq.size], d[at:at + td.size] = tq, td
    return q, d


def undense(q, d):
    """the inverse of dense()"""
    out = {}
    for size_id in range(4):
        nn = (4 << size_id) ** 2
        for lst in range(6):
            if size_id == 3 and lst not in (0, 1, 3):
                continue
            for rem in range(6):
                at = table_offset(size_id, lst, rem)
                out[(size_id, lst, rem)] = (np.array(q[at:at + nn], np.int32), np.array(d[at:at + nn], np.int32))
    return out


def lists_from_tables(tables):
    """the list coefficients and DC values behind processed tables: dequant[rem 0] / 40 -> (coeff, dc)"""
    coeff, dc = [], np.zeros((4, 6), np.int32)
    for size_id in range(4):
        n = 4 << size_id
        ratio = n // min(8, n)
        rows = []
        for lst in range(LIST_NUM[size_id]):
            dq = tables[(size_id, lst, 0)][1].reshape(n, n)
            assert (dq % 40 == 0).all()
            c = dq[::ratio, ::ratio] // 40
            if ratio > 1:
                dc[size_id][lst] = dq[0, 0] // 40
                c[0, 0] = dq[0, 1] // 40                               # (0, 1) reads coefficient 0 and is not the DC position
            rows.append(c.reshape(-1))
        coeff.append(np.array(rows, dtype=np.int32))
    return coeff, dc


def reference_default_tables():
    """the processed default lists as the compiled reference holds them after a call with sl = 1 -> {(size_id, list, rem): (q, d)}"""
    R.quant_batch(np.zeros((1, 16), np.int16), 4, 30, 0, 0, sl=1)
    return {(s, l, r): R.scaling_tables(s + 2, l, r, 4 << s) for s in range(4) for l in range(6) for r in range(6) if s < 3 or l in (0, 1, 3)}


def custom_lists(seed=4021):
    """a set in which U and V differ, some entries are 1..4 and the 16x16 / 32x32 DC values are distinct; the DC value of the inter
    32x32 list is 1 and of the intra one 2, which is where |coef| * factor passes 2^32 -> (coeff, dc)"""
    g = np.random.default_rng(seed)
    coeff = []
    for size_id in range(4):
        k = 16 if size_id == 0 else 64
        c = g.integers(8, 65, (LIST_NUM[size_id], k))
        small = g.random(c.shape) < 0.12
        c[small] = g.integers(1, 5, int(small.sum()))
        coeff.append(c.astype(np.int32))
    for size_id in range(3):
        for base in (0, 3):
            assert not np.array_equal(coeff[size_id][base + 1], coeff[size_id][base + 2])
    dc = np.zeros((4, 6), np.int32)
    dc[2] = (3, 21, 34, 5, 47, 12)
    dc[3, :2] = (2, 1)
    return coeff, dc


# ---------------------------------------------------------------- (2) the backend
class Listed:
    """base (ref_lib or oracle_lib) with scaling lists in quantize_residual_batch.  tables: process_lists(...) -> the oracle's table
    path; None -> the compiled reference's own default lists (sl = 1; base must be ref_lib).  log: one record per TU,
    (cu_is_intra, plane, n, has, dequant branch 1 / 2, max |coef| * factor >= 2^32, outputs change with V's own quantisation list)."""

    def __init__(self, base, tables=None, probe=False):
        assert tables is not None or base is R
        self.base, self.tables, self.probe, self.log = base, tables, probe, []

    def __getattr__(self, name):
        return getattr(self.base, name)

    def pick(self, n, qp, plane, cu_is_intra):
        size_id = {4: 0, 8: 1, 16: 2, 32: 3}[n]
        qps = scaled_qp(plane, qp)
        base = 0 if cu_is_intra else 3
        return size_id, base + (1 if plane else 0), base + plane, qps % 6, (1 if size_id + 5 > qps // 6 else 2)

    def quantize_residual_batch(self, ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra=0, signhide=0):
        size_id, lq, ld, rem, branch = self.pick(w, qp, color, cu_is_intra)
        if self.tables is None:
            out = R.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide, sl=1)
        else:
            out = O.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide,
                                            quant_coeff=self.tables[(size_id, lq, rem)][0], dequant_coeff=self.tables[(size_id, ld, rem)][1])
        count = len(out[2])
        big, swap = np.zeros(count, bool), np.zeros(count, bool)
        if self.probe and self.tables is not None:
            resid = (np.asarray(ref_in).reshape(count, -1).astype(np.int16) - np.asarray(pred_in).reshape(count, -1).astype(np.int16))
            coef = O.transform_batch("dst" if (cu_is_intra and w == 4 and color == 0) else "dct", w, resid).astype(np.int64)
            big = (np.abs(coef) * self.tables[(size_id, lq, rem)][0].astype(np.int64)).max(axis=1) >= 2 ** 32
            if color == 2:
                other = O.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide,
                                                  quant_coeff=self.tables[(size_id, ld, rem)][0], dequant_coeff=self.tables[(size_id, ld, rem)][1])
                swap = (other[0].reshape(count, -1) != out[0].reshape(count, -1)).any(axis=1) | (other[1].reshape(count, -1) != out[1].reshape(count, -1)).any(axis=1)
        self.log += [(int(bool(cu_is_intra)), int(color), int(w), int(out[2][i] != 0), branch, bool(big[i]), bool(swap[i])) for i in range(count)]
        return out


def coverage(log):
    """what the TUs of the fixture (the logs of the custom-list compositions, probe = True) fail to exercise -> list"""
    missing = []
    for intra, entry in ((0, "inter"), (1, "intra")):
        mine = [t for t in log if t[0] == intra]
        for (p, sizes) in ((0, (4, 8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
            for n in sizes:
                for has in (0, 1):
                    if not any(t[1] == p and t[2] == n and t[3] == has for t in mine):
                        missing.append("%s plane %d size %d has_coeffs %d" % (entry, p, n, has))
        for n in (4, 8, 16, 32):
            for branch in (1, 2):
                if not any(t[2] == n and t[3] == 1 and t[4] == branch for t in mine):
                    missing.append("%s size %d with coefficients in dequantisation branch %d" % (entry, n, branch))
        if not any(t[1] == 2 and t[6] for t in mine):
            missing.append("%s: a V TU whose outputs change with V's own quantisation list" % entry)
        if not any(t[5] for t in mine):
            missing.append("%s: a coefficient with |coef| * factor >= 2^32" % entry)
    return missing


# ---------------------------------------------------------------- (3) the pictures of tests/golden/scaling_list.npz
# (name, width, height, chroma, signhide, slice_is_intra, seed, intra_share, qp, lcu_qp or None, (col_bd, row_bd) of the intra entry or None)
FIXTURE_PICTURES = (
    ("hide", 128, 128, 1, 1, 0, 311, 0.45, 27, None, None),
    ("ragged", 200, 136, 1, 0, 0, 312, 0.4, 9, (22, 51, 48, 33, 44, 40, 22, 51, 37, 26, 30, 45), ((0, 2, 4), (0, 1, 3))),
    ("mono", 96, 72, 0, 0, 1, 313, 0.45, 32, None, None),
)
LIST_SETS = ("default", "custom")
# `ragged`: the full LCUs that are laid out by hand, LCU index -> (CU depth, tr_depth, quiet).  The CUs alternate inter / intra; the source
# of a loud CU is its prediction + 120 (inter) or a flat 235 (intra, DC mode), so that it keeps coefficients at any QP and its DC
# coefficient is near 15000 for a 32x32 TU; a quiet inter CU's source is its prediction and a quiet intra CU continues a flat 128 at
# the picture's corner, so that they keep none (the second quiet intra CU of the LCU has loud
# neighbours and keeps some).
# LCU 6 begins a tile of the intra entry: all intra, DC mode, a flat 128, which is what the tile's first TU predicts without neighbours
# and every later one from them -- intra TUs 16, 8 and (chroma) 4 wide without coefficients, whatever the lists.
DESIGNED = {0: (1, 1, True), 1: (1, 1, False), 2: (2, 2, False), 4: (3, 3, False), 5: (3, 4, False)}
FLAT_LCU = 6
CHAIN_START_QP = 30


def lcu_qp_array(pic):
    name, w, h, chroma, signhide, sii, seed, share, qp, lcu_qp, grid = pic
    lx, ly = QC.lcu_grid(w, h)
    return np.array(lcu_qp, np.int8) if lcu_qp is not None else np.full(lx * ly, qp, np.int8)


def design_lcu(cus, modes, src, pred, n_lcu, depth, trd, quiet):
    lx = (4 * cus.shape[1] + 63) // 64
    X0, Y0, size = 64 * (n_lcu % lx), 64 * (n_lcu // lx), 64 >> depth
    for y in range(Y0, Y0 + 64, size):
        for x in range(X0, X0 + 64, size):
            blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
            intra = ((x - X0) // size + (y - Y0) // size) % 2 == (0 if quiet else 1)
            cus[blk] = np.zeros((), CU_INFO)
            cus["depth"][blk], cus["tr_depth"][blk] = depth, trd
            cus["type"][blk], cus["mv_dir"][blk] = (IC.CU_INTRA, 0) if intra else (IC.CU_INTER, 1)
            modes[blk] = 1 if intra else XC.POISON_MODE
            loud = not quiet or (x - X0 >= 32 and y - Y0 < 32)
            for k in range(3):
                s = 1 if k else 0
                area = (slice(y >> s, (y + size) >> s), slice(x >> s, (x + size) >> s))
                pred[k][area] = 60 + 10 * k
                src[k][area] = (235 if loud else 128) if intra else pred[k][area] + (120 if loud else 0)


def flat_lcu(cus, modes, src, n_lcu):
    lx = (4 * cus.shape[1] + 63) // 64
    X0, Y0 = 64 * (n_lcu % lx), 64 * (n_lcu // lx)
    for (y0, depth) in ((Y0, 2), (Y0 + 32, 3)):                       # 16x16 CUs above, 8x8 CUs below
        blk = (slice(y0 // 4, y0 // 4 + 8), slice(X0 // 4, X0 // 4 + 16))
        cus[blk] = np.zeros((), CU_INFO)
        cus["type"][blk], cus["depth"][blk], cus["tr_depth"][blk] = IC.CU_INTRA, depth, depth
        modes[blk] = 1
    for k in range(3):
        s = 1 if k else 0
        src[k][Y0 >> s:(Y0 + 64) >> s, X0 >> s:(X0 + 64) >> s] = 128


def fixture_case(pic):
    """-> dict of the inputs.  Every record of `ragged` is an inter CU with motion or an intra CU (it also runs the chain up to
    deblocking, whose reference takes no blank record); the others hold blank and malformed records too"""
    name, w, h, chroma, signhide, sii, seed, share, qp, lcu_qp, grid = pic
    if name == "ragged":
        cus, _, modes = XC.make_map(w, h, seed, intra_share=share, blank_share=0.0, bad_share=0.0, edge_cu=False)
    else:
        cus, _, modes = XC.make_map(w, h, seed, intra_share=share, blank_share=0.08)
    pred = [None if p is None else np.array(p) for p in RC.smooth_planes(w, h, seed + 100, chroma)]
    inter_src = RC.make_source(pred, cus, seed + 200, chroma)
    intra_src = XC.make_planes(cus, seed + 300, chroma)[0]
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = [np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) if (k == 0 or chroma) else None for k in range(3)]
    if name == "ragged":
        for n_lcu, (depth, trd, quiet) in DESIGNED.items():
            design_lcu(cus, modes, src, pred, n_lcu, depth, trd, quiet)
        flat_lcu(cus, modes, src, FLAT_LCU)
    col_bd, row_bd = grid if grid else TC.one_tile(w, h)
    return {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": sii, "qp": qp,
            "lcu_qp": lcu_qp_array(pic), "per_lcu": lcu_qp is not None, "col_bd": list(col_bd), "row_bd": list(row_bd), "tiled": grid is not None,
            "src": tuple(src), "pred": tuple(pred), "cus": cus, "modes": modes}


def compose(case, B, grid=None):
    """-> (mid, full): what kvz_hip_inter_residual_frame_sl leaves over poisoned outputs (cbf_out cleared), and what
    kvz_hip_intra_recon_frame_sl makes of that.  B: a Listed backend; grid: (col_bd, row_bd), default the case's"""
    w, h, chroma = case["width"], case["height"], case["chroma"]
    col_bd, row_bd = grid or (case["col_bd"], case["row_bd"])
    init = QC.zero_outputs(w, h, chroma)
    mid = QC.compose_inter(case["src"], case["pred"], case["cus"], case["lcu_qp"], chroma, case["signhide"], case["slice_is_intra"], B=B, init=init)
    full = TC.compose_intra(case["src"], mid["rec"], mid["cus"], case["modes"], case["lcu_qp"], col_bd, row_bd, chroma, case["signhide"],
                            case["slice_is_intra"], B=B, init=(mid["coeff"], mid["cbf_out"], mid["costs"]))
    return mid, full


def compose_chain(case, B, base):
    """`ragged` without tiles: _sl inter -> _sl intra -> kvz_hip_cu_qp_frame -> kvz_hip_deblock_frame (per_cu_qp = 1)
    -> (records with qp, lcu_last_qp, deblocked planes)"""
    _, full = compose(case, B, TC.one_tile(case["width"], case["height"]))
    mapped, last = QC.set_cu_qps(full["cus"], full["cbf_out"], case["lcu_qp"], CHAIN_START_QP, 0)
    deb = base.deblock_frame(full["rec"][0], full["rec"][1], full["rec"][2], mapped, chain_deblock_params(case))
    return mapped, last, deb


def chain_deblock_params(case):
    return deblock_params(qp=CHAIN_START_QP, per_cu_qp=1, chroma=case["chroma"])


def _bytes(a):
    return a.view(np.uint8).reshape(a.shape + (20,))


def build_fixture(base=None, sets=LIST_SETS, default_tables=None, probe=True):
    """numeric arrays only -> (dict, missing coverage).  base: ref_lib (the default lists then go through the reference's own sl = 1
    path) or oracle_lib (they go through the oracle's table path with default_tables, the processed tables recorded from the reference)"""
    base = base or (R if R.available() else O)
    d, log = {}, []
    if default_tables is None:
        default_tables = reference_default_tables()
    d["default_quant"], d["default_dequant"] = dense(default_tables)
    coeff, dc = custom_lists()
    for size_id in range(4):
        d["custom_coeff_%d" % size_id] = coeff[size_id]
    d["custom_dc"] = dc
    custom = process_lists(coeff, dc)
    for pic in FIXTURE_PICTURES:
        case = fixture_case(pic)
        name, chroma = case["name"], case["chroma"]
        for k, n in enumerate("yuv"):
            if k == 0 or chroma:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = case["src"][k], case["pred"][k]
        d[name + "_cus"], d[name + "_modes"], d[name + "_lcu_qp"] = _bytes(case["cus"]), case["modes"], case["lcu_qp"]
        for which in sets:
            if which == "default":
                B = Listed(R) if base is R else Listed(O, default_tables)
            else:
                B = Listed(base, custom, probe)
            mid, full = compose(case, B)
            for stage, out in (("mid", mid), ("full", full)):
                tag = "%s_%s_%s" % (name, which, stage)
                for k, n in enumerate("yuv"):
                    if k == 0 or chroma:
                        d["%s_rec_%s" % (tag, n)], d["%s_coeff_%s" % (tag, n)] = out["rec"][k], out["coeff"][k]
                d[tag + "_cus"], d[tag + "_cbf_out"] = _bytes(out["cus"]), out["cbf_out"]
                d[tag + "_costs"] = out["costs"].view(np.uint32).reshape(case["cus"].shape + (6,))
            if which == "custom":
                log += B.log
                if name == "ragged":
                    mapped, last, deb = compose_chain(case, Listed(base, custom), base)
                    d["ragged_chain_cus"], d["ragged_chain_last"] = _bytes(mapped), last
                    for k, n in enumerate("yuv"):
                        d["ragged_chain_deb_" + n] = deb[k]
    return d, coverage(log) if (probe and "custom" in sets) else None


def load_case(z, pic):
    """the inputs of a picture from the fixture, as fixture_case returns them"""
    name, w, h, chroma, signhide, sii, seed, share, qp, lcu_qp, grid = pic
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    col_bd, row_bd = grid if grid else TC.one_tile(w, h)
    return {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": sii, "qp": qp,
            "lcu_qp": z[name + "_lcu_qp"], "per_lcu": lcu_qp is not None, "col_bd": list(col_bd), "row_bd": list(row_bd), "tiled": grid is not None,
            "src": planes("src"), "pred": planes("pred"), "cus": np.ascontiguousarray(z[name + "_cus"]).view(CU_INFO).reshape(h // 4, w // 4),
            "modes": z[name + "_modes"]}


def load_want(z, name, which, stage, chroma):
    tag = "%s_%s_%s" % (name, which, stage)
    planes = lambda kind: tuple(z["%s_%s_%s" % (tag, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    costs = np.ascontiguousarray(z[tag + "_costs"])
    cus = np.ascontiguousarray(z[tag + "_cus"])
    return {"rec": planes("rec"), "coeff": planes("coeff"), "cus": cus.view(CU_INFO).reshape(cus.shape[:2]), "cbf_out": z[tag + "_cbf_out"],
            "costs": costs.view(COST).reshape(costs.shape[:2])}


def load_tables(z, which):
    """-> (quant, dequant) packed"""
    if which == "default":
        return z["default_quant"], z["default_dequant"]
    return dense(process_lists([z["custom_coeff_%d" % s] for s in range(4)], z["custom_dc"]))


assert_outputs_equal = RC.assert_outputs_equal

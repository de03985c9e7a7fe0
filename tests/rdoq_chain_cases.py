"""Test-side reference of kvz_hip_inter_residual_frame_rdoq and kvz_hip_intra_recon_frame_rdoq: the pictures of tests/golden/lcu_qp.npz
(imported, not edited) through the two residual stages with the reference's quantiser at preset medium and slower -- kvz_rdoq where
width > 4 || !cfg.rdoq_skip, kvz_quant elsewhere (quant-generic.c:214-225).  The fixture tests/golden/rdoq_chain.npz holds the expected
outputs alone.  TEST INFRASTRUCTURE.

The composer here walks the TUs with inter_residual_cases.walk_tus / intra_recon_cases.walk_tus and hands every TU down with what the
existing compositions do not: its position (for the context set of its LCU) and the record at its own top-left SCU (for tr_depth).  A TU
is quantised by one of two routes:
  Reference  the compiled reference's own kvz_quantize_residual (tests/ref_quant_rdoq.py) on a fabricated state with cfg.rdoq_enable = 1:
             the reference picks the quantiser and derives tr_depth from the cu_info_t itself.  This route writes the fixture.
  Model      kvz_transform2d, kvz_dequant and kvz_itransform2d from the oracle (oracle_lib), the levels from tests/rdoq_model.py, the plain
             quantiser of a skipped 4x4 TU from the oracle: works without the reference, and takes the deliberate errors of MUTANTS.
Settings: six context sets made as in trskip_cabac_cases.context_sets, a lambda per set derived from a QP (SET_LAMBDA_QP; the LCUs' QPs
are those of lcu_qp.npz and have nothing to do with them, and set 4's lambda belongs to QP 12 on purpose, far from every QP it meets),
lcu_ctx by LCU position with one index beyond the table."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import rdoq_cases
import rdoq_model as M
import tile_chain_cases as TC
import trskip_cabac_cases as TCC
from patterns import CU_INFO

COST = RC.COST
N_SETS = TCC.N_SETS
SET_LAMBDA_QP = (27, 32, 22, 37, 12, 42)
BEYOND = 9                                                            # an index beyond the table: used as N_SETS - 1
# picture -> (rdoq_skip, lcu_ctx given, default scaling lists)
SETTINGS = {"ragged": (0, True, 0), "mono": (1, False, 0), "coarse": (0, True, 1), "deep": (0, True, 0)}
# the pictures: those of lcu_qp.npz, and `deep`, made here (own_inputs): two 64x64 CUs, inter and intra, whose records carry another
# tr_depth per quadrant, so that the record at a TU's top-left SCU and its CU's first record disagree -- no map of lcu_qp.npz has that.
# (name, width, height, chroma, signhide, slice_is_intra)
PICTURES = tuple(p[:6] for p in QC.FIXTURE_PICTURES) + (("deep", 128, 64, 1, 1, 0),)
TILE_GRID = {"ragged": ([0, 2, 4], [0, 1, 3])}                        # col_bd, row_bd of the one tiled run, in LCUs
MIN_DIFFERENT, MIN_HIDDEN, MIN_SET, MIN_LARGER = 20, 5, 5, 5


def context_sets():
    """(ranges uint16 [N_SETS], dumps uint8 [N_SETS, 184], lambdas float64 [N_SETS])"""
    ranges, dumps = TCC.context_sets()
    return ranges, dumps, np.array([rdoq_cases.lambda_of(q) for q in SET_LAMBDA_QP], dtype=np.float64)


def records(api):
    """(COEFF_CTX [N_SETS], RDOQ_STATE [N_SETS]) as the entries take them; states[].qp is not read by them and holds 0"""
    ranges, dumps, lambdas = context_sets()
    sets = np.array([api.coeff_ctx_from_dump(d, r) for d, r in zip(dumps, ranges)], dtype=api.COEFF_CTX)
    states = np.array([api.rdoq_state_from_dump(d, lam, 0) for d, lam in zip(dumps, lambdas)], dtype=api.RDOQ_STATE)
    return sets, states


def lcu_ctx_of(name, width, height):
    """uint16 [LCUs] in raster order or None: by LCU position, LCU 2 with an index beyond the table"""
    if not SETTINGS[name][1]:
        return None
    lx, ly = QC.lcu_grid(width, height)
    v = np.array([(5 * n + 1) % N_SETS for n in range(lx * ly)], dtype=np.uint16)
    v[min(2, v.size - 1)] = BEYOND
    return v


def set_of(lcu_ctx, lcu):
    return 0 if lcu_ctx is None else min(int(lcu_ctx[lcu]), N_SETS - 1)


def rdoq_tr_depth(rec):
    """quant-generic.c:218-219 on a record, clamped into 0..3 as the entries clamp it"""
    d = int(rec["tr_depth"]) - int(rec["depth"]) + (1 if int(rec["part_size"]) == XC.SIZE_NXN else 0)
    return min(max(d, 0), 3)


# ---------------------------------------------------------------- the two routes: one TU -> (rec [n, n], coeff [n * n], has)
class Reference:
    """the compiled reference's kvz_quantize_residual under cfg.rdoq_enable"""

    def __init__(self, rdoq_enable=1):
        import ref_quant_rdoq as Q
        self.Q, self.rdoq_enable = Q, rdoq_enable
        _, self.dumps, self.lambdas = context_sets()

    def __call__(self, t):
        r = t["record"]
        cu = (int(r["type"]), int(r["depth"]), int(r["tr_depth"]), int(r["part_size"]))
        return self.Q.quantize_residual(t["src"], t["pred"], t["n"], t["plane"], t["scan"], cu, t["qp"], self.lambdas[t["set"]], self.dumps[t["set"]],
                                        rdoq_enable=self.rdoq_enable, rdoq_skip=t["skip"], signhide=t["signhide"], default_lists=t["lists"],
                                        slice_is_intra=t["slice_is_intra"])


MUTANTS = ("rdoq-on-skipped-4x4", "plain-quantiser-for-8x8", "tr-depth-without-nxn", "tr-depth-of-the-cus-first-record", "set-of-the-next-lcu",
           "lambda-of-the-lcus-qp", "type-2-for-luma", "diagonal-scan-in-the-intra-stage", "has-coeffs-of-the-plain-levels")


class Model:
    """oracle transforms and dequantisation around tests/rdoq_model.py; mutant: one deliberate error of MUTANTS, or None.
    tables: {0: (quant, err_scale, None), 1: (quant, err_scale, dequant)} packed, for flat and default lists.  The last mutant takes
    has_coeffs from the levels the plain quantiser would leave (so the reconstruction runs, and the flags are set, where RDOQ left no
    level): running the reconstruction itself on zero levels returns the prediction and could not show."""

    def __init__(self, tables, mutant=None, plain=False, cache=None):
        assert mutant is None or mutant in MUTANTS
        self.tables, self.mutant, self.plain = tables, mutant, plain
        _, self.dumps, self.lambdas = context_sets()
        self.cache = {} if cache is None else cache

    def _table(self, which, lists, log2, plane, intra, qp, own_plane=False):
        qps = M.scaled_qp(2 if plane else 0, qp)
        lst = (0 if intra else 3) + ((plane if own_plane else 1) if plane else 0)
        at = M.table_offset(log2 - 2, lst, qps % 6)
        return np.ascontiguousarray(self.tables[lists][which][at:at + (1 << (2 * log2))])

    def plain_levels(self, t, coef, log2, intra):
        q = self._table(0, 1, log2, t["plane"], intra, t["qp"]) if t["lists"] else None
        return O.quant_batch(coef[None], t["n"], t["qp"], 2 if t["plane"] else 0, t["scan"], t["slice_is_intra"], t["signhide"], int(intra),
                             quant_coeff=q)[0]

    def __call__(self, t):
        n, plane, m = t["n"], t["plane"], self.mutant
        log2 = n.bit_length() - 1
        intra = int(t["record"]["type"]) == IC.CU_INTRA
        res = (t["src"].astype(np.int16) - t["pred"].astype(np.int16)).reshape(-1)
        kind = "dst" if (intra and n == 4 and plane == 0) else "dct"
        coef = O.transform_batch(kind, n, res[None])[0]
        use_rdoq = (n > 4 or not t["skip"] or m == "rdoq-on-skipped-4x4") and not (m == "plain-quantiser-for-8x8" and n == 8) and not self.plain
        if use_rdoq:
            rec = t["cu_record"] if m == "tr-depth-of-the-cus-first-record" else t["record"]
            trd = rdoq_tr_depth(rec)
            if m == "tr-depth-without-nxn":
                trd = min(max(int(rec["tr_depth"]) - int(rec["depth"]), 0), 3)
            s = t["next_set"] if m == "set-of-the-next-lcu" else t["set"]
            lam = rdoq_cases.lambda_of(t["qp"]) if m == "lambda-of-the-lcus-qp" else float(self.lambdas[s])
            type_ = 2 if (plane or m == "type-2-for-luma") else 0
            scan = 0 if (m == "diagonal-scan-in-the-intra-stage" and intra) else t["scan"]
            key = (coef.tobytes(), n, type_, scan, int(rec["type"]), trd, t["qp"], lam, s, t["signhide"], t["lists"])
            if key not in self.cache:
                quant, err = self.tables[t["lists"]][0], self.tables[t["lists"]][1]
                self.cache[key] = np.array(M.rdoq(coef.tolist(), n, type_, scan, int(rec["type"]), trd, t["qp"], lam, self.dumps[s].tolist(), quant, err,
                                                  signhide=t["signhide"]), dtype=np.int16)
            levels = self.cache[key]
        else:
            levels = self.plain_levels(t, coef, log2, intra)
        has = int(levels.any())
        if m == "has-coeffs-of-the-plain-levels" and use_rdoq:
            has = int(self.plain_levels(t, coef, log2, intra).any())
        if not has:
            return np.array(t["pred"], dtype=np.uint8), levels, 0
        dq = self._table(2, 1, log2, plane, intra, t["qp"], own_plane=True) if t["lists"] else None
        back = O.dequant_batch(levels[None], n, t["qp"], (0, 2, 3)[plane], int(intra), dequant_coeff=dq)
        res2 = O.transform_batch("i" + kind, n, back)[0].astype(np.int64)
        val = ((res2 + t["pred"].reshape(-1).astype(np.int64) + 32768) % 65536) - 32768          # int16_t val (quant-generic.c:255)
        return np.clip(val, 0, 255).astype(np.uint8).reshape(n, n), levels, has


def model_tables(rdoq_z, sl_z):
    """the packed tables of the Model from tests/golden/rdoq.npz (quant and err_scale, flat and default) and scaling_list.npz (dequant)"""
    return {0: (rdoq_z["quant"][0], rdoq_z["err_scale"][0], None), 1: (rdoq_z["quant"][1], rdoq_z["err_scale"][1], sl_z["default_dequant"])}


# ---------------------------------------------------------------- the composer
def _outputs(cus, init, width, height, chroma):
    if init is None:
        n = ((width + 63) // 64) * ((height + 63) // 64)
        init = (tuple(np.zeros((n, 1024 if k else 4096), np.int16) if (k == 0 or chroma) else None for k in range(3)),
                np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, COST))
    return [None if c is None else np.array(c) for c in init[0]], np.array(init[1]), np.array(init[2])


def _store(t, r, c, has, src_blk, coeff, cus, cbf_out, costs, lcus_x):
    p, x, y, n, cu_x, cu_y = t["plane"], t["x"], t["y"], t["n"], t["cu_x"], t["cu_y"]
    sh = 1 if p else 0
    z = RC.xy_to_zorder(32 if p else 64, (x & 63) >> sh, (y & 63) >> sh)
    coeff[p][(y >> 6) * lcus_x + (x >> 6), z:z + n * n] = c
    span = (2 * n if p else n) // 4
    scu = (slice(y // 4, y // 4 + span), slice(x // 4, x // 4 + span))
    if p == 0:
        cus["cbf_y"][scu] = has
    cbf_out[scu] |= (has << p)
    d, dz = src_blk.astype(np.int64) - r, src_blk.astype(np.int64) - t["pred"]
    f = "_c" if p else "_y"
    costs["ssd" + f][cu_y // 4, cu_x // 4] += np.uint32((d * d).sum())
    costs["zero_ssd" + f][cu_y // 4, cu_x // 4] += np.uint32((dz * dz).sum())
    costs["coeff_abs" + f][cu_y // 4, cu_x // 4] += np.uint32(np.abs(c.astype(np.int64)).sum())


def _tu(name, cus, lcu_qp, lcu_ctx, width, p, x, y, n, cu_x, cu_y, scan, signhide, slice_is_intra):
    lx = (width + 63) // 64
    lcu = (y >> 6) * lx + (x >> 6)
    skip, _, lists = SETTINGS[name]
    n_lcu = lcu_qp.size
    return {"plane": p, "x": x, "y": y, "n": n, "cu_x": cu_x, "cu_y": cu_y, "scan": scan, "qp": QC.qp_at(lcu_qp, width, x, y), "record": cus[y // 4, x // 4],
            "cu_record": cus[cu_y // 4, cu_x // 4], "set": set_of(lcu_ctx, lcu), "next_set": set_of(lcu_ctx, (lcu + 1) % n_lcu) if lcu_ctx is not None else 1,
            "skip": skip, "lists": lists, "signhide": int(signhide), "slice_is_intra": int(slice_is_intra)}


def compose_inter(name, src, pred, cus, lcu_qp, quantize, chroma=1, signhide=0, slice_is_intra=0, init=None):
    """the outputs of kvz_hip_inter_residual_frame_rdoq as RC.compose returns them; "tus": the TU descriptions with "levels" and "has" """
    height, width = src[0].shape
    lcu_qp = np.asarray(lcu_qp).reshape(-1)
    lcu_ctx = lcu_ctx_of(name, width, height)
    rec = [None if p is None or (k and not chroma) else np.array(p, dtype=np.uint8) for k, p in enumerate(pred)]
    cus = np.array(cus)
    records = np.array(cus)                                           # the records as the call finds them: cbf_y is written, never read
    coeff, cbf_out, costs = _outputs(cus, init, width, height, chroma)
    for (x, y, size) in RC.inter_cus(cus, width, height):
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    tus = []
    for (p, x, y, n, cu_x, cu_y) in RC.walk_tus(cus, width, height, chroma):
        t = _tu(name, records, lcu_qp, lcu_ctx, width, p, x, y, n, cu_x, cu_y, 0, signhide, slice_is_intra)
        sh = 1 if p else 0
        blk = (slice(y >> sh, (y >> sh) + n), slice(x >> sh, (x >> sh) + n))
        t["src"], t["pred"] = np.array(src[p][blk]), np.array(rec[p][blk])
        r, c, has = quantize(t)
        rec[p][blk] = r
        _store(t, r, c, has, t["src"], coeff, cus, cbf_out, costs, (width + 63) // 64)
        t["levels"], t["has"] = c, has
        tus.append(t)
    return {"rec": tuple(rec), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": tus}


def compose_intra(name, src, rec, cus, modes, lcu_qp, quantize, chroma=1, signhide=0, slice_is_intra=0, init=None, grid=None, B=None):
    """the outputs of kvz_hip_intra_recon_frame_rdoq as XC.compose returns them.  grid = (col_bd, row_bd): a tiled picture -- a TU takes
    its neighbours from its tile alone, as a picture of its own (tile_chain_cases); set and QP stay those of the picture's LCU"""
    B = B or XC.backend()
    height, width = src[0].shape
    lcu_qp = np.asarray(lcu_qp).reshape(-1)
    lcu_ctx = lcu_ctx_of(name, width, height)
    n_planes = 3 if chroma else 1
    full = [np.array(p, dtype=np.uint8) for p in rec[:n_planes]]
    work = [np.ascontiguousarray(p[:height >> (1 if k else 0), :width >> (1 if k else 0)]) for k, p in enumerate(full)]
    cus = np.array(cus)
    records = np.array(cus)
    coeff, cbf_out, costs = _outputs(cus, init, width, height, chroma)
    for (x, y, size) in XC.intra_cus(cus, width, height):
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    rects = TC.tiles(width, height, *grid) if grid else [(0, 0, width, height, None)]
    tus = []
    for (p, x, y, n, cu_x, cu_y, mode, scan, leaf) in XC.walk_tus(cus, modes, width, height, chroma):
        t = _tu(name, records, lcu_qp, lcu_ctx, width, p, x, y, n, cu_x, cu_y, scan, signhide, slice_is_intra)
        sh = 1 if p else 0
        x0, y0, x1, y1 = next(r[:4] for r in rects if r[0] <= x < r[2] and r[1] <= y < r[3])
        tile = np.ascontiguousarray(work[p][y0 >> sh:y1 >> sh, x0 >> sh:x1 >> sh])
        ref = XC.build_ref(B, n.bit_length() - 1, p, tile, x1 - x0, y1 - y0, x - x0, y - y0)
        blk = (slice(y >> sh, (y >> sh) + n), slice(x >> sh, (x >> sh) + n))
        t["src"], t["pred"] = np.array(src[p][blk]), np.array(XC.predict(B, ref, n.bit_length() - 1, mode, p).reshape(n, n), dtype=np.uint8)
        r, c, has = quantize(t)
        work[p][blk] = r
        _store(t, r, c, has, t["src"], coeff, cus, cbf_out, costs, (width + 63) // 64)
        t["levels"], t["has"], t["mode"], t["leaf"] = c, has, mode, leaf
        tus.append(t)
    for k in range(n_planes):
        full[k][:work[k].shape[0], :work[k].shape[1]] = work[k]
    pad = [None] * (3 - n_planes)
    return {"rec": tuple(full + pad), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": tus}


def compose_chain(name, case, quantize, chroma, signhide, slice_is_intra, grid=None):
    """inter stage, then intra stage, over poisoned outputs (cbf_out cleared once by the caller) -> (mid, full)"""
    src, pred, cus, modes, lcu_qp = case
    height, width = src[0].shape
    init = QC.zero_outputs(width, height, chroma)
    mid = compose_inter(name, src, pred, cus, lcu_qp, quantize, chroma, signhide, slice_is_intra, init=init)
    full = compose_intra(name, src, mid["rec"], mid["cus"], modes, lcu_qp, quantize, chroma, signhide, slice_is_intra,
                         init=(mid["coeff"], mid["cbf_out"], mid["costs"]), grid=grid)
    return mid, full


# `mono` of lcu_qp.npz holds 14 TUs wider than 4, of which RDOQ changes two: it cannot meet the conditions below under rdoq_skip.  So
# this module gives that picture inputs of its own -- the same size and format, a map with more intra CUs, louder sources and lower QPs --
# which the fixture stores (mono_in_*).
OWN_INPUTS = {"mono": (700, (22, 27, 17, 32)), "deep": (903, (24, 29))}   # picture -> (seed, lcu_qp)
DEEP_TR_DEPTH = ((1, 2), (3, 2))                                      # tr_depth of the records of the four 32x32 quadrants of a 64x64 CU


def deep_inputs(pic):
    """`deep`: LCU 0 one inter CU, LCU 1 one intra CU, both 64x64 (depth 0); the tree splits by the tr_depth of each node's own record"""
    name, w, h, chroma = pic[:4]
    seed, lcu_qp = OWN_INPUTS[name]
    g = np.random.default_rng(seed)
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    modes = np.full(cus.shape + (2,), XC.POISON_MODE, np.uint8)
    cus["mv_dir"] = 1
    cus["type"][:, :16], cus["type"][:, 16:] = IC.CU_INTER, IC.CU_INTRA
    for j in range(2):
        for i in range(2):
            for lcu in range(2):
                cus["tr_depth"][8 * j:8 * j + 8, 16 * lcu + 8 * i:16 * lcu + 8 * i + 8] = DEEP_TR_DEPTH[j][i]
    modes[:, 16:, 0] = np.kron(np.array(XC.LISTED_MODES)[g.integers(0, len(XC.LISTED_MODES), (8, 8))], np.ones((2, 2), dtype=np.int64))
    modes[:, 16:, 1] = np.kron(np.array((0, 26, 10, 1, 34))[g.integers(0, 5, (2, 2))], np.ones((8, 8), dtype=np.int64))
    pred = RC.smooth_planes(w, h, seed + 100, chroma)
    src = []
    for k in range(3):
        a = pred[k].astype(np.int64)
        amp = np.kron(np.array((2, 4, 7, 12))[g.integers(0, 4, (a.shape[0] // 8, a.shape[1] // 8))], np.ones((8, 8), dtype=np.int64))
        src.append(np.clip(a + np.rint((g.random(a.shape) * 2 - 1) * amp), 0, 255).astype(np.uint8))
    return tuple(src), pred, cus, modes, np.array(lcu_qp, np.int8)


def own_inputs(pic):
    """(src, pred, cus, modes, lcu_qp) made here for a picture of OWN_INPUTS"""
    name, w, h, chroma = pic[:4]
    if name == "deep":
        return deep_inputs(pic)
    seed, lcu_qp = OWN_INPUTS[name]
    cus, _, modes = XC.make_map(w, h, seed, intra_share=0.5, blank_share=0.0)
    pred = RC.smooth_planes(w, h, seed + 100, chroma)
    inter_src = RC.make_source(pred, cus, seed + 200, chroma, amps=(3, 8, 14, 24, 48))
    intra_src = XC.make_planes(cus, seed + 300, chroma, amps=(2, 8, 16, 40))[0]
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = tuple(np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) if (k == 0 or chroma) else None for k in range(3))
    return src, pred, cus, modes, np.array(lcu_qp, np.int8)


def store_inputs(d, name, case, chroma):
    src, pred, cus, modes, lcu_qp = case
    for k, n in enumerate("yuv"):
        if k == 0 or chroma:
            d["%s_in_src_%s" % (name, n)], d["%s_in_pred_%s" % (name, n)] = src[k], pred[k]
    d[name + "_in_cus"], d[name + "_in_modes"], d[name + "_in_lcu_qp"] = _bytes(cus), modes, lcu_qp


def load_inputs(z, pic, fixture=None):
    """(src, pred, cus, modes, lcu_qp) of a picture: of tests/golden/lcu_qp.npz (z), or, for a picture of OWN_INPUTS, what
    tests/golden/rdoq_chain.npz stores (fixture; None: made afresh)"""
    name, chroma = pic[0], pic[3]
    if name in OWN_INPUTS:
        if fixture is None:
            return own_inputs(pic)
        planes = lambda kind: tuple(fixture["%s_in_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
        cus = np.ascontiguousarray(fixture[name + "_in_cus"])
        return planes("src"), planes("pred"), cus.view(CU_INFO).reshape(cus.shape[:2]), fixture[name + "_in_modes"], np.asarray(fixture[name + "_in_lcu_qp"])
    src, pred, cus, modes, lcu_qp, _ = QC.load_fixture_case(z, name, chroma)
    return src, pred, cus, modes, np.asarray(lcu_qp)


# ---------------------------------------------------------------- the conditions the fixture must meet
def _differs(a, b):
    return not np.array_equal(a, b)


def conditions(name, chroma, stages, variants):
    """why the picture cannot tell the entries from wrong ones -> list.  stages: {"inter": tus, "intra": tus} of the composition;
    variants: the same TUs quantised otherwise, {"plain" / "nohide" / "set0": {"inter": [levels], "intra": [levels]}}"""
    missing = []
    for stage, tus in stages.items():
        plain = variants["plain"][stage]
        diff = [(t["plane"], t["n"]) for t, v in zip(tus, plain) if _differs(t["levels"], v)]
        if len(diff) < MIN_DIFFERENT:
            missing.append("%s %s: %d TUs differ from the plain quantiser, %d wanted" % (name, stage, len(diff), MIN_DIFFERENT))
        # every width and plane the picture has (with rdoq_skip the 4x4 TUs keep the plain quantiser)
        have = {(t["plane"], t["n"]) for t in tus if not (t["skip"] and t["n"] == 4)}
        for key in sorted(have - set(diff)):
            missing.append("%s %s: no TU of plane %d width %d differs from the plain quantiser" % ((name, stage) + key))
    everything = stages["inter"] + stages["intra"]
    if name == "ragged":
        hidden = sum(_differs(t["levels"], v) for st in stages for t, v in zip(stages[st], variants["nohide"][st]))
        if hidden < MIN_HIDDEN:
            missing.append("ragged: sign hiding changed %d TUs, %d wanted" % (hidden, MIN_HIDDEN))
        by_set = sum(_differs(t["levels"], v) for st in stages for t, v in zip(stages[st], variants["set0"][st]))
        if by_set < MIN_SET:
            missing.append("ragged: %d TUs change with set 0, %d wanted" % (by_set, MIN_SET))
    if name == "mono":
        small = [(t, v) for st in stages for t, v in zip(stages[st], variants["plain"][st]) if t["n"] == 4]
        if not small or any(_differs(t["levels"], v) for t, v in small):
            missing.append("mono: a 4x4 luma TU differs from the _sl composition, or there is none")
        larger = sum(_differs(t["levels"], v) for st in stages for t, v in zip(stages[st], variants["plain"][st]) if t["n"] > 4)
        if larger < MIN_LARGER:
            missing.append("mono: %d larger TUs differ from the _sl composition, %d wanted" % (larger, MIN_LARGER))
    if name == "deep":
        moved = sum(_differs(t["levels"], v) for st in stages for t, v in zip(stages[st], variants["first"][st]))
        if moved < 1:
            missing.append("deep: no TU changes when tr_depth is taken from its CU's first record")
        return missing
    for p in ((0, 1) if chroma else (0,)):
        depths = {rdoq_tr_depth(t["record"]) > 0 for t in everything if (t["plane"] != 0) == bool(p)}
        if depths != {False, True}:
            missing.append("%s: tr_depth 0 and above 0 in %s" % (name, "chroma" if p else "luma"))
    return missing


def _bytes(a):
    return a.view(np.uint8).reshape(a.shape + (20,))


def store(d, tag, out, chroma):
    for k, n in enumerate("yuv"):
        if k == 0 or chroma:
            d["%s_rec_%s" % (tag, n)], d["%s_coeff_%s" % (tag, n)] = out["rec"][k], out["coeff"][k]
    d[tag + "_cus"], d[tag + "_cbf_out"] = _bytes(out["cus"]), out["cbf_out"]
    d[tag + "_costs"] = out["costs"].view(np.uint32).reshape(out["cus"].shape + (6,))


def load_want(z, tag, chroma):
    planes = lambda kind: tuple(z["%s_%s_%s" % (tag, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    costs, cus = np.ascontiguousarray(z[tag + "_costs"]), np.ascontiguousarray(z[tag + "_cus"])
    return {"rec": planes("rec"), "coeff": planes("coeff"), "cus": cus.view(CU_INFO).reshape(cus.shape[:2]), "cbf_out": z[tag + "_cbf_out"],
            "costs": costs.view(COST).reshape(costs.shape[:2])}


def build_fixture(inputs_z):
    """the expected outputs alone, from the compiled reference: per picture the outputs after the inter stage (_mid) and after the intra
    stage (_full), for `ragged` also after the tiled intra stage (_tiled).  -> (dict, what the conditions miss)"""
    d, missing = {}, []
    ref, ref_plain = Reference(1), Reference(0)
    for pic in PICTURES:
        name, w, h, chroma, signhide, slice_is_intra = pic
        case = load_inputs(inputs_z, pic)
        mid, full = compose_chain(name, case, ref, chroma, signhide, slice_is_intra)
        stages = {"inter": mid["tus"], "intra": full["tus"]}
        variants = {"plain": {st: [ref_plain(t)[1] for t in tus] for st, tus in stages.items()}}
        if name == "ragged":
            variants["nohide"] = {st: [ref(dict(t, signhide=0))[1] for t in tus] for st, tus in stages.items()}
            variants["set0"] = {st: [ref(dict(t, set=0))[1] for t in tus] for st, tus in stages.items()}
        if name == "deep":
            variants["first"] = {st: [ref(dict(t, record=t["cu_record"]))[1] for t in tus] for st, tus in stages.items()}
        missing += conditions(name, chroma, stages, variants)
        store(d, name + "_mid", mid, chroma)
        store(d, name + "_full", full, chroma)
        if name in OWN_INPUTS:
            store_inputs(d, name, case, chroma)
        if name in TILE_GRID:
            _, tiled = compose_chain(name, case, ref, chroma, signhide, slice_is_intra, grid=TILE_GRID[name])
            if all(np.array_equal(a, b) for a, b in zip(tiled["rec"], full["rec"])):
                missing.append(name + ": the tile grid changes no pixel")
            store(d, name + "_tiled", tiled, chroma)
    return d, missing

"""Test-side reference of the transform-skip entries of the picture chain: kvz_hip_inter_residual_frame_ts and
kvz_hip_intra_recon_frame_ts.

Two parts.  (1) Skipping: a backend that forwards everything to ref_lib or oracle_lib except quantize_residual_batch, which for a 4x4
luma TU runs the backend's function with use_trskip 0 and 1, prices both trials with the backend's pixels_calc_ssd and coeff_abs_sum and
keeps one.  Handed as `B` to the existing compositions (lcu_qp_cases.compose_inter, tile_chain_cases.compose_intra, which walk the trees
of inter_residual_cases / intra_recon_cases) it gives the expected outputs, and its log gives the tr_skip map and what coverage() reads.
The decision -- decide() below, ten lines -- is a RESTATEMENT of kvz_quantize_residual_trskip (transform.c:244-266) with the estimate of
kvz_get_coeff_cost below fast_residual_cost_limit (rdo.c:219-220): the compiled harness has no entry for kvz_quantize_residual_trskip.
Everything under the decision is the reference's own functions.  Scaling lists: the backend picks the TU's tables by the rule of
scaling_list_cases.Listed, whose quantize_residual_batch has no use_trskip to forward.  (2) The pictures of tests/golden/trskip.npz.
TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import lcu_qp_cases as QC
import oracle_lib as O
import ref_lib as R
import scaling_list_cases as SL
import tile_chain_cases as TC
from patterns import CU_INFO, deblock_params

COST = RC.COST
POISON_SKIP = 0x7B
COEFF_COST_QP_FACTOR, COEFF_COST_BIAS = 0.044407704, 0.557323653     # rdo.c:44-45
MASK32 = 0xFFFFFFFF


# ---------------------------------------------------------------- (1) the backend
def coeff_cost(abs_sum, qp):
    """kvz_get_coeff_cost with state->qp < fast_residual_cost_limit (rdo.c:219-220); Python floats are C doubles, and every operation
    rounds on its own"""
    return int(abs_sum * (qp * COEFF_COST_QP_FACTOR + COEFF_COST_BIAS) + 0.5) & MASK32


def decide(ssd, abs_sum, qp, bit_cost):
    """transform.c:244-266 -> (1 if the skipped trial is kept, (noskip.cost, skip.cost)); ssd, abs_sum: (transformed, skipped)"""
    cost = [(ssd[t] + coeff_cost(abs_sum[t], qp) * (bit_cost & MASK32)) & MASK32 for t in (0, 1)]
    return (0 if cost[0] <= cost[1] else 1), tuple(cost)


class Skipping:
    """base (ref_lib or oracle_lib) with the two trials of transform skip in quantize_residual_batch.
    bit_cost: one int, or {clamped LCU QP: int} where it follows the LCU (the compositions hand the TU's QP down, not its position).
    lists: None = flat; "default" = the compiled reference's own default lists (sl = 1; base must be ref_lib); a dict of processed tables
    (scaling_list_cases.process_lists) = the oracle's table path.
    probe: the bit costs under which every decision is taken again for the log.  force: {index into the log: choice} overrides.
    log: one dict per 4x4 luma TU, in call order."""

    def __init__(self, base, bit_cost, lists=None, probe=(), force=None):
        assert lists != "default" or base is R
        self.base, self.bit_cost, self.lists, self.probe, self.force, self.log = base, bit_cost, lists, tuple(probe), dict(force or {}), []
        self.pick = SL.Listed(O, {}).pick

    def __getattr__(self, name):
        return getattr(self.base, name)

    def cost_of(self, qp):
        v = self.bit_cost[qp] if isinstance(self.bit_cost, dict) else self.bit_cost
        return max(int(v), 0)

    def trial(self, ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide, use_trskip):
        if self.lists is None:
            return self.base.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide, use_trskip)
        if self.lists == "default":
            return R.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide, use_trskip, sl=1)
        size_id, lq, ld, rem, _ = self.pick(w, qp, color, cu_is_intra)
        return O.quantize_residual_batch(ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide, use_trskip,
                                         quant_coeff=self.lists[(size_id, lq, rem)][0], dequant_coeff=self.lists[(size_id, ld, rem)][1])

    def quantize_residual_batch(self, ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra=0, signhide=0):
        args = (ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide)
        if w != 4 or color != 0:
            return self.trial(*args, 0)
        both = [self.trial(*args, t) for t in (0, 1)]
        ref_b, pred_b = np.asarray(ref_in, np.uint8).reshape(-1, 16), np.asarray(pred_in, np.uint8).reshape(-1, 16)
        rec, coeff, has = (np.array(a) for a in both[0])
        rec, coeff = rec.reshape(-1, 16), coeff.reshape(-1, 16)
        bit_cost = self.cost_of(qp)
        for i in range(len(has)):
            r = [np.ascontiguousarray(both[t][0].reshape(-1, 16)[i]) for t in (0, 1)]
            c = [np.ascontiguousarray(both[t][1].reshape(-1, 16)[i]) for t in (0, 1)]
            ssd = [int(self.base.pixels_calc_ssd(np.ascontiguousarray(ref_b[i]), 0, r[t], 0, 4, 4, 4)) for t in (0, 1)]
            sab = [int(self.base.coeff_abs_sum(c[t])) for t in (0, 1)]
            choice, cost = decide(ssd, sab, qp, bit_cost)
            choice = self.force.get(len(self.log), choice)
            if choice:
                rec[i], coeff[i], has[i] = r[1], c[1], both[1][2][i]
            edge = bool((r[0].reshape(4, 4)[:, 3] != r[1].reshape(4, 4)[:, 3]).any() or (r[0].reshape(4, 4)[3] != r[1].reshape(4, 4)[3]).any())
            self.log.append({"intra": int(bool(cu_is_intra)), "qp": int(qp), "bit_cost": bit_cost, "skip": choice, "cost": cost,
                             "has": (int(both[0][2][i] != 0), int(both[1][2][i] != 0)), "edge": edge, "pred": pred_b[i].tobytes(),
                             "flips": len({decide(ssd, sab, qp, b)[0] for b in self.probe}) > 1})
        return rec, coeff, has


def tables_of(lists, base, default_tables=None):
    """the `lists` argument of Skipping for a picture: None, or the default lists through `base`"""
    if lists is None:
        return None
    if base is R:
        return "default"
    return default_tables


def compose(case, base, default_tables=None, bit_cost=None, probe=(), force_intra=None, grid=None):
    """-> (mid, full): what kvz_hip_inter_residual_frame_ts leaves over zeroed outputs, and what kvz_hip_intra_recon_frame_ts makes of
    that; each with "tr_skip" [h / 4, w / 4] (POISON_SKIP where the entries write nothing; full continues mid's) and "log", the
    Skipping records of its 4x4 luma TUs with "x", "y" added.  bit_cost: default the case's (per LCU where the case says so)."""
    w, h, chroma = case["width"], case["height"], case["chroma"]
    col_bd, row_bd = grid or (case["col_bd"], case["row_bd"])
    lists = tables_of(case["lists"], base, default_tables)
    if bit_cost is None:
        bit_cost = case["bit_cost"]
    if np.ndim(bit_cost):
        q = QC.clip_qp(case["lcu_qp"]).reshape(-1)
        bc = {int(v): int(b) for v, b in zip(q, np.asarray(bit_cost).reshape(-1))}
        assert all(bc[int(v)] == int(b) for v, b in zip(q, np.asarray(bit_cost).reshape(-1))), "a bit cost per QP"
        bit_cost = bc
    init = QC.zero_outputs(w, h, chroma)
    # inter: lcu_qp_cases.compose_inter runs the whole picture once per distinct QP and stitches by LCU; so does the map
    B = Skipping(base, bit_cost, lists, probe)
    mid = QC.compose_inter(case["src"], case["pred"], case["cus"], case["lcu_qp"], chroma, case["signhide"], case["slice_is_intra"], B=B, init=init)
    pos = [(t[1], t[2]) for t in RC.walk_tus(case["cus"], w, h, chroma) if t[0] == 0 and t[3] == 4]
    runs = sorted({int(v) for v in QC.clip_qp(case["lcu_qp"]).reshape(-1)})
    assert len(B.log) == len(pos) * len(runs)
    skip = np.full(case["cus"].shape, POISON_SKIP, np.uint8)
    mid["log"] = []
    for i, (x, y) in enumerate(pos):
        rec = dict(B.log[runs.index(QC.qp_at(case["lcu_qp"], w, x, y)) * len(pos) + i], x=x, y=y)
        assert rec["qp"] == QC.qp_at(case["lcu_qp"], w, x, y) and not rec["intra"]
        skip[y // 4, x // 4] = rec["skip"]
        mid["log"].append(rec)
    mid["tr_skip"] = skip
    # intra: one walk in coding order, tile by tile; the log follows the walk's summary
    B = Skipping(base, bit_cost, lists, probe, force_intra)
    full = TC.compose_intra(case["src"], mid["rec"], mid["cus"], case["modes"], case["lcu_qp"], col_bd, row_bd, chroma, case["signhide"],
                            case["slice_is_intra"], B=B, init=(mid["coeff"], mid["cbf_out"], mid["costs"]))
    pos = [(t[5], t[6]) for t in full["tus"] if t[0] == 0 and t[1] == 4]
    assert len(B.log) == len(pos)
    skip = np.array(skip)
    full["log"] = []
    for (x, y), rec in zip(pos, B.log):
        assert rec["intra"] and rec["qp"] == QC.qp_at(case["lcu_qp"], w, x, y)
        skip[y // 4, x // 4] = rec["skip"]
        full["log"].append(dict(rec, x=x, y=y))
    full["tr_skip"] = skip
    return mid, full


def neighbour_follows(case, base, full, default_tables=None):
    """is there an intra TU whose right or lower neighbour's prediction changes because skip won?  Taken literally: the first intra TU
    that kept the skipped trial, whose two trials differ in the last column or row and whose right or lower neighbour is a later 4x4
    TU, is forced to the transformed trial in a second composition, and the neighbour's prediction is compared."""
    log = full["log"]
    at = {(r["x"], r["y"]): i for i, r in enumerate(log)}
    for i, r in enumerate(log):
        if not (r["skip"] and r["edge"]):
            continue
        near = [at[p] for p in ((r["x"] + 4, r["y"]), (r["x"], r["y"] + 4)) if at.get(p, -1) > i]
        if not near:
            continue
        _, other = compose(case, base, default_tables, force_intra={i: 0})
        assert other["log"][i]["skip"] == 0
        if any(other["log"][j]["pred"] != log[j]["pred"] for j in near):
            return True
    return False


def coverage(logs, followed):
    """what the 4x4 luma TUs of the fixture fail to exercise -> list.  logs: {picture: the records of both entries}; followed: the
    answer of neighbour_follows for a picture with intra CUs"""
    missing = []
    every = [r for log in logs.values() for r in log]
    for name, log in logs.items():
        n = [sum(1 for r in log if r["skip"] == t) for t in (0, 1)]
        for t, what in ((0, "transformed"), (1, "skipped")):
            if n[t] == 0 or 10 * n[t] < len(log):
                missing.append("%s: the %s trial is kept in %d of %d TUs" % (name, what, n[t], len(log)))
    if not any(r["skip"] and r["has"][1] for r in every):
        missing.append("a skipped winner with coefficients")
    if not any(r["cost"][0] == r["cost"][1] and not r["skip"] for r in every):
        missing.append("a tie that goes to the transformed trial")
    if not any(r["has"][0] != r["has"][1] for r in every):
        missing.append("a TU whose two trials disagree about has_coeffs")
    if not followed:
        missing.append("an intra TU whose right or lower neighbour's prediction changes because skip won")
    if not any(r["flips"] for r in every):
        missing.append("a TU whose decision flips between two bit costs of the fixture")
    return missing


# ---------------------------------------------------------------- (2) the pictures of tests/golden/trskip.npz
def lambda_bit_cost(qp):
    """(int)(lambda + 0.5) with the lambda of a P slice without rate control, 0.57 * 2^((qp - 12) / 3)"""
    return int(0.57 * 2.0 ** ((qp - 12) / 3.0) + 0.5)


MIXED_LCU_QP = (22, 37, 27, 32, 17, 42)
# (name, width, height, chroma, signhide, slice_is_intra, seed, intra_share, qp, lcu_qp or None, (col_bd, row_bd) or None, default lists)
FIXTURE_PICTURES = (
    ("inter", 72, 72, 1, 1, 0, 511, 0.0, 27, None, None, False),
    ("intra", 72, 72, 1, 1, 1, 512, 1.0, 27, None, None, False),
    ("mixed", 136, 72, 1, 0, 0, 513, 0.5, 30, MIXED_LCU_QP, ((0, 1, 3), (0, 1, 2)), True),
    ("mono", 72, 72, 0, 0, 0, 514, 0.5, 32, None, None, False),
)
CHAIN_START_QP = 30
LUMA_MODES = (0, 1, 2, 10, 18, 26, 34, 8, 12, 24, 28)                # planar, DC, diagonal scans, 6..14 vertical scan, 22..30 horizontal scan


def picture_bit_cost(pic):
    """the bit cost of the fixture's run: (int)(lambda + 0.5) of the picture's QP, or of every LCU's"""
    lcu_qp = pic[9]
    return np.array([lambda_bit_cost(q) for q in lcu_qp], np.int32) if lcu_qp is not None else lambda_bit_cost(pic[8])


def probe_costs():
    """every bit cost the fixture uses"""
    out = set()
    for pic in FIXTURE_PICTURES:
        out |= set(np.atleast_1d(picture_bit_cost(pic)).tolist())
    return tuple(sorted(out))


def make_map(w, h, seed, intra_share):
    """every record an inter CU with motion or an intra CU (the chain's deblocking reference takes no blank record).  Per 16x16 area:
    one 16x16 CU with a 16x16 TU, or four 8x8 CUs, each with one 8x8 TU or -- most of them -- four 4x4 luma TUs and one 4x4 TU per
    chroma plane.  An area that crosses the picture's edge holds the 8x8 CUs that fit.  -> (cus, modes)"""
    g = np.random.default_rng(seed)
    cus = np.zeros((h // 4, w // 4), CU_INFO)
    modes = np.full(cus.shape + (2,), XC.POISON_MODE, np.uint8)

    def cu(x, y, size, depth, trd):
        blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
        intra = g.random() < intra_share
        cus["depth"][blk], cus["tr_depth"][blk] = depth, trd
        cus["type"][blk], cus["mv_dir"][blk] = (IC.CU_INTRA, 0) if intra else (IC.CU_INTER, 1)
        if intra:
            m = g.choice(LUMA_MODES, (size // 4, size // 4)) if trd == 4 else np.full((size // 4, size // 4), g.choice(LUMA_MODES))
            if trd == 4:
                cus["part_size"][blk] = XC.SIZE_NXN
            modes[blk + (0,)] = m
            modes[blk + (1,)] = int(m[0, 0]) if g.random() < 0.5 else int(g.choice((0, 26, 10, 1, 34)))
    for y in range(0, h, 16):
        for x in range(0, w, 16):
            if x + 16 <= w and y + 16 <= h and g.random() < 0.15:
                cu(x, y, 16, 2, 2)
                continue
            for dy in (0, 8):
                for dx in (0, 8):
                    if x + dx + 8 <= w and y + dy + 8 <= h:
                        cu(x + dx, y + dy, 8, 3, 4 if g.random() < 0.8 else 3)
    return cus, modes


def make_planes(w, h, seed, chroma):
    """-> (src, pred).  The prediction of the inter CUs is smooth; the source is, per 4x4 luma block, one of: the prediction (no
    coefficients either way), the prediction plus gentle noise (the transform pays), a two-level, text-like pattern of sharp edges
    over the prediction (transform skip pays), or a single pixel step.  The intra CUs predict from their neighbours, so the same
    source serves them."""
    g = np.random.default_rng(seed)
    pred = [None if p is None else np.array(p[:h >> (k > 0), :w >> (k > 0)]) for k, p in enumerate(RC.smooth_planes(w, h, seed + 1, chroma))]
    src = []
    for k in range(3 if chroma else 1):
        ph, pw = pred[k].shape
        kind = np.kron(g.integers(0, 8, ((ph + 3) // 4, (pw + 3) // 4)), np.ones((4, 4), np.int64))[:ph, :pw]
        noise = g.integers(-6, 7, (ph, pw))
        level = np.kron(g.choice((18, 40, 90), ((ph + 3) // 4, (pw + 3) // 4)), np.ones((4, 4), np.int64))[:ph, :pw]
        text = np.where(g.random((ph, pw)) < 0.4, level, 0)
        step = np.where((np.arange(pw)[None, :] % 4 == 1) & (np.arange(ph)[:, None] % 4 == 2), level, 0)
        d = np.select([kind == 0, kind <= 2, kind <= 5, kind == 6], [0, noise, text, step], default=noise // 2 + text // 4)
        src.append(np.clip(pred[k].astype(np.int64) + d, 0, 255).astype(np.uint8))
    none = [None] * (0 if chroma else 2)
    return tuple(src + none), tuple(pred + none)


def fixture_case(pic):
    name, w, h, chroma, signhide, sii, seed, share, qp, lcu_qp, grid, lists = pic
    cus, modes = make_map(w, h, seed, share)
    src, pred = make_planes(w, h, seed + 100, chroma)
    lx, ly = QC.lcu_grid(w, h)
    col_bd, row_bd = grid if grid else TC.one_tile(w, h)
    return {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": sii, "qp": qp,
            "lcu_qp": np.array(lcu_qp, np.int8) if lcu_qp is not None else np.full(lx * ly, qp, np.int8), "per_lcu": lcu_qp is not None,
            "col_bd": list(col_bd), "row_bd": list(row_bd), "tiled": grid is not None, "lists": "default" if lists else None,
            "bit_cost": picture_bit_cost(pic), "src": src, "pred": pred, "cus": cus, "modes": modes}


def compose_chain(case, base, default_tables=None):
    """`mixed`: _ts inter -> _ts intra -> kvz_hip_cu_qp_frame_tiles -> kvz_hip_deblock_frame_tiles (per_cu_qp = 1)
    -> (records with qp, lcu_last_qp, deblocked planes)"""
    _, full = compose(case, base, default_tables)
    mapped, last = TC.set_cu_qps(full["cus"], full["cbf_out"], case["lcu_qp"], CHAIN_START_QP, case["col_bd"], case["row_bd"], 0)
    deb = TC.deblock(full["rec"], mapped, chain_deblock_params(case), case["col_bd"], case["row_bd"], base)
    return mapped, last, deb


def chain_deblock_params(case):
    return deblock_params(qp=CHAIN_START_QP, per_cu_qp=1, chroma=case["chroma"])


def _bytes(a):
    return a.view(np.uint8).reshape(a.shape + (20,))


def store(d, tag, out, chroma):
    for k, n in enumerate("yuv"):
        if k == 0 or chroma:
            d["%s_rec_%s" % (tag, n)], d["%s_coeff_%s" % (tag, n)] = out["rec"][k], out["coeff"][k]
    d[tag + "_cus"], d[tag + "_cbf_out"], d[tag + "_tr_skip"] = _bytes(out["cus"]), out["cbf_out"], out["tr_skip"]
    d[tag + "_costs"] = out["costs"].view(np.uint32).reshape(out["cus"].shape + (6,))


def build_fixture(base=None, default_tables=None, probe=True):
    """numeric arrays only -> (dict, missing coverage or None).  base: ref_lib (the default lists then go through the reference's own
    sl = 1 path) or oracle_lib (they go through the oracle's table path with default_tables, the processed tables of
    tests/golden/scaling_list.npz, recorded from the reference)"""
    base = base or (R if R.available() else O)
    d, logs, followed = {}, {}, False
    costs = probe_costs() if probe else ()
    for pic in FIXTURE_PICTURES:
        case = fixture_case(pic)
        name, chroma = case["name"], case["chroma"]
        for k, n in enumerate("yuv"):
            if k == 0 or chroma:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = case["src"][k], case["pred"][k]
        d[name + "_cus"], d[name + "_modes"], d[name + "_lcu_qp"] = _bytes(case["cus"]), case["modes"], case["lcu_qp"]
        d[name + "_bit_cost"] = np.atleast_1d(np.asarray(case["bit_cost"], np.int32))
        mid, full = compose(case, base, default_tables, probe=costs)
        store(d, name + "_mid", mid, chroma)
        store(d, name + "_full", full, chroma)
        logs[name] = mid["log"] + full["log"]
        if probe and name == "intra":
            followed = neighbour_follows(case, base, full, default_tables)
        if name == "mixed":
            mapped, last, deb = compose_chain(case, base, default_tables)
            d["mixed_chain_cus"], d["mixed_chain_last"] = _bytes(mapped), last
            for k, n in enumerate("yuv"):
                d["mixed_chain_deb_" + n] = deb[k]
    return d, (coverage(logs, followed) if probe else None)


def load_case(z, pic):
    """the inputs of a picture from the fixture, as fixture_case returns them"""
    name, w, h, chroma, signhide, sii, seed, share, qp, lcu_qp, grid, lists = pic
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    col_bd, row_bd = grid if grid else TC.one_tile(w, h)
    bc = z[name + "_bit_cost"]
    return {"name": name, "width": w, "height": h, "chroma": chroma, "signhide": signhide, "slice_is_intra": sii, "qp": qp,
            "lcu_qp": z[name + "_lcu_qp"], "per_lcu": lcu_qp is not None, "col_bd": list(col_bd), "row_bd": list(row_bd), "tiled": grid is not None,
            "lists": "default" if lists else None, "bit_cost": np.array(bc) if lcu_qp is not None else int(bc[0]),
            "src": planes("src"), "pred": planes("pred"), "cus": np.ascontiguousarray(z[name + "_cus"]).view(CU_INFO).reshape(h // 4, w // 4),
            "modes": z[name + "_modes"]}


def load_want(z, name, stage, chroma):
    tag = "%s_%s" % (name, stage)
    planes = lambda kind: tuple(z["%s_%s_%s" % (tag, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    costs = np.ascontiguousarray(z[tag + "_costs"])
    cus = np.ascontiguousarray(z[tag + "_cus"])
    return {"rec": planes("rec"), "coeff": planes("coeff"), "cus": cus.view(CU_INFO).reshape(cus.shape[:2]), "cbf_out": z[tag + "_cbf_out"],
            "costs": costs.view(COST).reshape(costs.shape[:2]), "tr_skip": z[tag + "_tr_skip"]}


def assert_outputs_equal(got, want, what="", chroma=1):
    RC.assert_outputs_equal(got, want, what, chroma)
    np.testing.assert_array_equal(got["tr_skip"], want["tr_skip"], err_msg=what + ": tr_skip_out")

"""The pictures of tests/golden/trskip_cabac.npz: the small pictures of tests/trskip_cases.py (imported, not edited), composed as there --
the compiled reference's kvz_quantize_residual twice per 4x4 luma TU -- but with kvz_get_coeff_cost's own rule for the price of a trial
(rdo.c:208-222): at or above fast_limit the count of the reference's counting coder (tests/ref_coeff_cost.py) on the LCU's context set,
below it the estimate.  What kvz_hip_inter_residual_frame_ts_cabac and kvz_hip_intra_recon_frame_ts_cabac must leave.  TEST INFRASTRUCTURE.

The compositions of trskip_cases hand a TU's QP down, not its position, so a picture's set index per LCU is a function of the LCU's QP
(SET_OF_QP): `mixed` has six QPs and so six different indices, one of them beyond the table (used as the last set); the pictures with one
QP have one index, and `inter` passes lcu_ctx == NULL (set 0)."""
import numpy as np

import coeff_cabac_model as M
import lcu_qp_cases as QC
import ref_coeff_cost as RCC
import trskip_cases as T

N_SETS = 6
# picture -> (fast_limit, lcu_ctx given, bit cost or None: the picture's own of trskip_cases).  `mixed`: QPs 17 22 27 below, 32 37 42 at
# or above the limit; `mono`: the QP equals the limit, which prices with CABAC (>=); `inter`: the default limit 0
PRICING = {"inter": (0, False, None), "intra": (20, True, None), "mixed": (30, True, None), "mono": (32, True, None)}
SET_OF_QP = {17: 4, 22: 1, 27: 3, 32: 2, 37: 9, 42: 5, 30: 0}        # 9: beyond the table, used as N_SETS - 1
MIN_DIFFERENT = 20


def context_sets():
    """(ranges [N_SETS], dumps [N_SETS, 184]) as a host would dump them, and the records"""
    g = np.random.default_rng(20240612)
    return g.integers(256, 511, N_SETS).astype(np.uint16), g.integers(0, 126, (N_SETS, 184)).astype(np.uint8)


def records(api):
    ranges, dumps = context_sets()
    return np.array([api.coeff_ctx_from_dump(d, r) for d, r in zip(dumps, ranges)], dtype=api.COEFF_CTX)


def lcu_ctx_of(case):
    """uint16 [LCUs] or None"""
    if not PRICING[case["name"]][1]:
        return None
    return np.array([SET_OF_QP[int(q)] for q in QC.clip_qp(case["lcu_qp"]).reshape(-1)], dtype=np.uint16)


def count(coeff16, scan, set_index, signhide, use_reference=True):
    """get_coeff_cabac_cost of one trial: type 0, trskip_enable 1, lossless 0, the transform_skip_flag bin 0 (rdo.c:188-194)"""
    ranges, dumps = context_sets()
    s = min(set_index, N_SETS - 1)
    if use_reference and RCC.available():
        return RCC.coeff_cabac_cost(coeff16, 4, 0, scan, int(ranges[s]), dumps[s], signhide, 1, 0, 0)[0]
    return M.count_bits(np.asarray(coeff16).tolist(), 4, 0, scan, 0, int(ranges[s]), dumps[s].tolist(), signhide, 1, 0)


class Pricing(T.Skipping):
    """T.Skipping with kvz_get_coeff_cost's rule for the price of a trial.  The log gains "estimate": the choice under the estimate."""
    fast_limit, with_ctx, use_reference = 0, False, True

    def quantize_residual_batch(self, ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra=0, signhide=0):
        args = (ref_in, pred_in, w, qp, color, scan_order_, cu_is_intra, slice_is_intra, signhide)
        if w != 4 or color != 0:
            return self.trial(*args, 0)
        both = [self.trial(*args, t) for t in (0, 1)]
        ref_b, pred_b = np.asarray(ref_in, np.uint8).reshape(-1, 16), np.asarray(pred_in, np.uint8).reshape(-1, 16)
        rec, coeff, has = (np.array(a) for a in both[0])
        rec, coeff = rec.reshape(-1, 16), coeff.reshape(-1, 16)
        bit_cost = self.cost_of(qp)
        set_index = SET_OF_QP[int(qp)] if self.with_ctx else 0
        for i in range(len(has)):
            r = [np.ascontiguousarray(both[t][0].reshape(-1, 16)[i]) for t in (0, 1)]
            c = [np.ascontiguousarray(both[t][1].reshape(-1, 16)[i]) for t in (0, 1)]
            ssd = [int(self.base.pixels_calc_ssd(np.ascontiguousarray(ref_b[i]), 0, r[t], 0, 4, 4, 4)) for t in (0, 1)]
            sab = [int(self.base.coeff_abs_sum(c[t])) for t in (0, 1)]
            estimate, _ = T.decide(ssd, sab, qp, bit_cost)
            if qp >= self.fast_limit:                           # rdo.c:214
                price = [count(c[t], scan_order_, set_index, int(bool(signhide)), self.use_reference) for t in (0, 1)]
                cost = tuple((ssd[t] + price[t] * (bit_cost & T.MASK32)) & T.MASK32 for t in (0, 1))
                choice = 0 if cost[0] <= cost[1] else 1             # transform.c:260
            else:
                choice, cost = T.decide(ssd, sab, qp, bit_cost)
            if choice:
                rec[i], coeff[i], has[i] = r[1], c[1], both[1][2][i]
            self.log.append({"intra": int(bool(cu_is_intra)), "qp": int(qp), "bit_cost": bit_cost, "skip": choice, "cost": cost, "estimate": estimate,
                             "cabac": int(qp >= self.fast_limit), "has": (int(both[0][2][i] != 0), int(both[1][2][i] != 0)), "edge": False,
                             "pred": pred_b[i].tobytes(), "flips": False})
        return rec, coeff, has


def compose(case, base, default_tables=None, fast_limit=None, use_reference=True):
    """T.compose with the pricing rule -> (mid, full); fast_limit: default the picture's"""
    limit, with_ctx, bit_cost = PRICING[case["name"]]

    def make(*a, **kw):
        p = Pricing(*a, **kw)
        p.fast_limit, p.with_ctx, p.use_reference = (limit if fast_limit is None else fast_limit), with_ctx, use_reference
        return p
    saved = T.Skipping
    T.Skipping = make
    try:
        return T.compose(case, base, default_tables, bit_cost=bit_cost)
    finally:
        T.Skipping = saved


def coverage(name, mid, full):
    """why the picture cannot tell the entries from wrong ones, or None"""
    for stage, log in (("inter", mid["log"]), ("intra", full["log"])):
        if not log:
            continue
        if {r["skip"] for r in log} != {0, 1}:
            return "%s: one winner only among the %s TUs" % (name, stage)
    different = sum(1 for r in mid["log"] + full["log"] if r["skip"] != r["estimate"])
    if different < MIN_DIFFERENT:
        return "%s: %d TUs decided differently under CABAC pricing, %d wanted" % (name, different, MIN_DIFFERENT)
    return None


def build_fixture(base, default_tables=None):
    """the expected outputs alone: the inputs are those of tests/golden/trskip.npz -> (dict, why not or None)"""
    d = {}
    for pic in T.FIXTURE_PICTURES:
        case = T.fixture_case(pic)
        name = case["name"]
        mid, full = compose(case, base, default_tables)
        why = coverage(name, mid, full)
        if why:
            return d, why
        T.store(d, name + "_mid", mid, case["chroma"])
        T.store(d, name + "_full", full, case["chroma"])
        d[name + "_decided"] = np.array([[r["x"], r["y"], r["intra"], r["skip"], r["estimate"], r["cabac"]] for r in mid["log"] + full["log"]], np.int32)
    ranges, dumps = context_sets()
    d["ranges"], d["dumps"] = ranges, dumps
    return d, None

"""Test-side reference of the per-LCU-QP entries: kvz_hip_inter_residual_frame_qp, kvz_hip_intra_recon_frame_qp and
kvz_hip_cu_qp_frame.

Inter: an inter TU lies inside one LCU and depends on nothing else, so the expected outputs are inter_residual_cases.compose run once
per distinct QP and stitched by LCU.  Intra: TUs depend on their neighbours across LCUs, so there is a walk of its own in coding order
with the QP looked up per TU, built from intra_recon_cases.walk_tus / build_ref / predict and the backend's quantize_residual_batch --
the compiled reference (ref_lib) where it was built, else the oracle (oracle_lib).

set_cu_qps (encoderstate.c:550-609) is a static function without a harness entry.  set_cu_qps() below is a RESTATEMENT of it, with
kvz_get_cu_ref_qp (encoderstate.c:1408-1430) and is_last_cu_in_qg (encoderstate.h:332-342), as the reference's own recursive walk over
the records; the kernel's rule ("CUs before the first coded CU get last_qp") has a different shape and is not used here.
TEST INFRASTRUCTURE."""
import numpy as np

import inter_recon_cases as IC
import inter_residual_cases as RC
import intra_recon_cases as XC
import oracle_lib as O
import ref_lib as R
from patterns import CU_INFO

COST = RC.COST


def backend():
    return R if R.available() else O


def lcu_grid(width, height):
    return (width + 63) // 64, (height + 63) // 64


def clip_qp(lcu_qp):
    """what the entries do to the array: any value is brought into 0..51"""
    return np.clip(np.asarray(lcu_qp, dtype=np.int64), 0, 51)


def qp_at(lcu_qp, width, x, y):
    return int(clip_qp(lcu_qp).reshape(-1)[(y >> 6) * ((width + 63) // 64) + (x >> 6)])


# ---------------------------------------------------------------- inter: one composition per distinct QP, stitched by LCU
def _tu_positions(cus, width, height, chroma):
    """(plane, x, y, n) of the TUs in the order of the "tus" summary of RC.compose: grouped by (plane, n), the walk's order inside"""
    groups = {}
    for t in RC.walk_tus(cus, width, height, chroma):
        groups.setdefault((t[0], t[3]), []).append(t)
    return [(t[0], t[1], t[2], t[3]) for key in sorted(groups) for t in groups[key]]


def compose_inter(src, pred, cus, lcu_qp, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None, many=False):
    """the outputs of kvz_hip_inter_residual_frame_qp as RC.compose returns them; "tus": [(plane, n, has, qp)]"""
    height, width = src[0].shape
    lx, ly = lcu_grid(width, height)
    q = clip_qp(lcu_qp).reshape(ly, lx)
    runs = {int(v): RC.compose(src, pred, cus, int(v), chroma, signhide, slice_is_intra, B=B, init=init, many=many) for v in np.unique(q)}
    out = {k: (tuple(None if p is None else np.array(p) for p in v) if k in ("rec", "coeff") else np.array(v))
           for k, v in next(iter(runs.values())).items() if k != "tus"}
    for j in range(ly):
        for i in range(lx):
            r = runs[int(q[j, i])]
            for k in range(3 if chroma else 1):
                u = 32 if k else 64
                out["rec"][k][j * u:(j + 1) * u, i * u:(i + 1) * u] = r["rec"][k][j * u:(j + 1) * u, i * u:(i + 1) * u]
                out["coeff"][k][j * lx + i] = r["coeff"][k][j * lx + i]
            blk = (slice(16 * j, 16 * j + 16), slice(16 * i, 16 * i + 16))
            for k in ("cus", "cbf_out", "costs"):
                out[k][blk] = r[k][blk]
    pos = _tu_positions(cus, width, height, chroma)
    tus = []
    for n_tu, (p, x, y, n) in enumerate(pos):
        v = int(q[y >> 6, x >> 6])
        t = runs[v]["tus"][n_tu]
        assert (t[0], t[1]) == (p, n)
        tus.append((p, n, t[2], v))
    out["tus"] = tus
    return out


# ---------------------------------------------------------------- intra: the walk of XC.compose with the QP of the TU's LCU
def compose_intra(src, rec, cus, modes, lcu_qp, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None):
    """the outputs of kvz_hip_intra_recon_frame_qp as XC.compose returns them; "tus": [(plane, n, has, mode, scan, x, y, leaf, signhide, qp)]"""
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
    for (x, y, size) in XC.intra_cus(cus, width, height):
        cbf_out[y // 4:(y + size) // 4, x // 4:(x + size) // 4] = 0
        costs[y // 4, x // 4] = 0
    summary = []
    for (p, x, y, n, cu_x, cu_y, mode, scan, leaf) in XC.walk_tus(cus, modes, width, height, chroma):
        sh = 1 if p else 0
        log2 = {4: 2, 8: 3, 16: 4, 32: 5}[n]
        px, py = x >> sh, y >> sh
        qp = qp_at(lcu_qp, width, x, y)
        ref = XC.build_ref(B, log2, p, work[p], width, height, x, y)
        pred = XC.predict(B, ref, log2, mode, p).reshape(n, n)
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
        summary.append((p, n, has, mode, scan, x, y, leaf, int(signhide), qp))
    for k in range(n_planes):
        full[k][:work[k].shape[0], :work[k].shape[1]] = work[k]
    pad = [None] * (3 - n_planes)
    return {"rec": tuple(full + pad), "coeff": tuple(coeff), "cus": cus, "cbf_out": cbf_out, "costs": costs, "tus": summary}


# ---------------------------------------------------------------- set_cu_qps, restated
def set_cu_qps(cus, cbf, lcu_qp, start_qp, chain_lcus=0, max_qp_delta_depth=0):
    """RESTATEMENT of set_cu_qps (encoderstate.c:550-609) over every LCU of the picture, in raster order, as
    encoder_state_worker_encode_lcu calls it (encoderstate.c:735-741: prev_qp = -1, last_qp carried from LCU to LCU, state->frame->QP at
    the start of a chain, :729).  -> (records with qp written, last_qp on entry to each LCU as int8).

    Before the walk every record carries the QP of its LCU (cur_cu->qp = state->qp, search.c:451).  cbf: one byte per SCU; where the
    reference asks cbf_is_set_any of the CU's record (or of the records of its TUs), this asks whether any byte inside the CU is set:
    the reference's flags are propagated up to the CU's depth, a plain byte per SCU is not."""
    cus = np.array(cus)
    hs, ws = cus.shape
    height, width = 4 * hs, 4 * ws
    lx, ly = lcu_grid(width, height)
    q = clip_qp(lcu_qp).reshape(ly, lx)
    cus["qp"] = np.kron(q, np.ones((16, 16), dtype=np.int64))[:hs, :ws]
    depth_of = np.minimum(cus["depth"].astype(int), 3)
    state = {"last": int(start_qp), "prev": -1}

    def ref_qp(x, y):
        # kvz_get_cu_ref_qp (encoderstate.c:1408-1430)
        qg = 64 >> min(max_qp_delta_depth, int(depth_of[y // 4, x // 4]))
        xq, yq = x & ~(qg - 1), y & ~(qg - 1)
        a = int(cus["qp"][yq // 4, (xq - 1) // 4]) if xq % 64 > 0 else state["last"]
        b = int(cus["qp"][(yq - 1) // 4, xq // 4]) if yq % 64 > 0 else state["last"]
        return (a + b + 1) >> 1

    def is_last_cu_in_qg(x, y, depth):
        # encoderstate.h:332-342
        if max_qp_delta_depth < 0:
            return False
        cw, qg = 64 >> depth, 64 >> max_qp_delta_depth
        right, bottom = x + cw, y + cw
        return (right % qg == 0 or right >= width) and (bottom % qg == 0 or bottom >= height)

    def walk(x, y, depth):
        if x >= width or y >= height:
            return
        cw = 64 >> depth
        if depth <= max_qp_delta_depth:
            state["prev"] = -1
        if depth_of[y // 4, x // 4] > depth:
            d = cw >> 1
            walk(x, y, depth + 1)
            walk(x + d, y, depth + 1)
            walk(x, y + d, depth + 1)
            walk(x + d, y + d, depth + 1)
            return
        area = (slice(y // 4, min((y + cw) // 4, hs)), slice(x // 4, min((x + cw) // 4, ws)))
        cbf_found = state["prev"] >= 0 or bool(np.asarray(cbf)[area].any())
        if cbf_found:
            state["prev"] = qp = int(cus["qp"][y // 4, x // 4])
        else:
            qp = ref_qp(x, y)
        cus["qp"][area] = qp
        if is_last_cu_in_qg(x, y, depth):
            state["last"] = int(cus["qp"][y // 4, x // 4])

    last_in = np.zeros(lx * ly, np.int8)
    for j in range(ly):
        for i in range(lx):
            n = j * lx + i
            if n == 0 or (chain_lcus and n % chain_lcus == 0):
                state["last"] = int(start_qp)
            last_in[n] = state["last"]
            state["prev"] = -1
            walk(64 * i, 64 * j, 0)
    return cus, last_in


def leaf_cus(cus):
    """[(x, y, size)] of the leaves of set_cu_qps' walk, in coding order (for building and checking maps)"""
    hs, ws = cus.shape
    depth_of = np.minimum(cus["depth"].astype(int), 3)
    out = []

    def walk(x, y, depth):
        if x >= 4 * ws or y >= 4 * hs:
            return
        cw = 64 >> depth
        if depth_of[y // 4, x // 4] > depth:
            for (dx, dy) in ((0, 0), (cw // 2, 0), (0, cw // 2), (cw // 2, cw // 2)):
                walk(x + dx, y + dy, depth + 1)
        else:
            out.append((x, y, cw))
    for Y0 in range(0, 4 * hs, 64):
        for X0 in range(0, 4 * ws, 64):
            walk(X0, Y0, 0)
    return out


# ---------------------------------------------------------------- the known answers of the QP map
KNOWN_W, KNOWN_H, KNOWN_START = 200, 136, 40
KNOWN_LCU_QP = tuple(range(20, 32))                                   # LCU n has QP 20 + n; 4 x 3 LCUs, ragged right and bottom
# per LCU: (depth of its records, index in coding order of its first coded CU or None).  Depth 1: four 32x32 CUs; the ragged LCUs hold
# 8x8 CUs (depth 3): a column of eight at the right edge, a row of eight at the bottom, a single one in the corner.
KNOWN_LCUS = ((1, 0), (1, 2), (1, None), (3, 2),
              (1, None), (1, None), (1, 3), (3, None),
              (3, 3), (3, None), (3, 0), (3, 0))
# last_qp on entry to each LCU, worked out by hand: one chain over the picture / a chain per LCU row
KNOWN_LAST_ONE_CHAIN = (40, 20, 21, 21, 23, 23, 23, 26, 26, 28, 28, 30)
KNOWN_LAST_ROW_CHAINS = (40, 20, 21, 21, 40, 40, 40, 26, 40, 28, 28, 30)
KNOWN_CASES = ("an LCU whose first CU is coded", "one whose first coded CU is in the middle", "one with none", "two uncoded LCUs in a row",
               "a chain start", "chain_lcus 0 against row chains", "ragged right and bottom LCUs")


def known_map():
    """-> (cus, cbf, expected qp per SCU for one chain, the same for row chains).  The expected maps are written from the two hand-made
    tables above by the plain statement of the result: the CUs before the first coded one carry last_qp, the others the LCU's QP."""
    w, h = KNOWN_W, KNOWN_H
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    cus["type"] = IC.CU_INTER
    cbf = np.zeros(cus.shape, np.uint8)
    lx, ly = lcu_grid(w, h)
    for n, (depth, first) in enumerate(KNOWN_LCUS):
        cus["depth"][16 * (n // lx):16 * (n // lx) + 16, 16 * (n % lx):16 * (n % lx) + 16] = depth
    leaves = leaf_cus(cus)
    want = [np.zeros(cus.shape, np.uint8), np.zeros(cus.shape, np.uint8)]
    for n, (depth, first) in enumerate(KNOWN_LCUS):
        mine = [c for c in leaves if (c[1] >> 6) * lx + (c[0] >> 6) == n]
        assert len(mine) > 1 or n == 11, "each LCU holds several CUs"
        for i, (x, y, s) in enumerate(mine):
            area = (slice(y // 4, min((y + s) // 4, h // 4)), slice(x // 4, min((x + s) // 4, w // 4)))
            if first is not None and i == first:
                cbf[area][-1, -1] = 1 + (n % 7)                        # one SCU of the CU, not its first: any SCU counts
            for k, last in enumerate((KNOWN_LAST_ONE_CHAIN, KNOWN_LAST_ROW_CHAINS)):
                want[k][area] = KNOWN_LCU_QP[n] if first is not None and i >= first else last[n]
    return cus, cbf, want[0], want[1]


# ---------------------------------------------------------------- the pictures of tests/golden/lcu_qp.npz
# (name, width, height, chroma, signhide, slice_is_intra, seed, intra_share, start_qp, lcu_qp)
FIXTURE_PICTURES = (
    ("ragged", 200, 136, 1, 1, 0, 71, 0.4, 30, (0, 51, 22, 37, 27, 32, 43, 30, 17, 46, 25, 35)),
    ("mono", 96, 72, 0, 0, 0, 72, 0.4, 26, (20, 33, 45, 28)),
    ("coarse", 256, 128, 1, 0, 0, 98, 0.5, 34, (10, 48, 24, 40, 51, 4, 34, 18)),
)
PARAMS_QP = 7                                                         # params->qp of the _qp calls: ignored when the array is given


def coarse_map(w, h, seed, intra_share):
    """a map of large CUs only, for the large transforms: LCU n holds CUs of depth n % 3 (64, 32 or 16 wide), each inter or intra, with
    tr_depth = max(1, depth) -> (cus, modes)"""
    g = np.random.default_rng(seed)
    cus = np.zeros((h // 4, w // 4), dtype=CU_INFO)
    modes = np.full(cus.shape + (2,), XC.POISON_MODE, np.uint8)
    lx = (w + 63) // 64
    for Y0 in range(0, h, 64):
        for X0 in range(0, w, 64):
            depth = ((Y0 >> 6) * lx + (X0 >> 6)) % 3
            size = 64 >> depth
            for y in range(Y0, Y0 + 64, size):
                for x in range(X0, X0 + 64, size):
                    blk = (slice(y // 4, (y + size) // 4), slice(x // 4, (x + size) // 4))
                    cus["depth"][blk], cus["tr_depth"][blk], cus["mv_dir"][blk] = depth, max(1, depth), 1
                    cus["type"][blk] = IC.CU_INTRA if g.random() < intra_share else IC.CU_INTER
                    if cus["type"][y // 4, x // 4] == IC.CU_INTRA:
                        modes[blk + (0,)] = int(XC.LISTED_MODES[g.integers(0, len(XC.LISTED_MODES))])
                        modes[blk + (1,)] = int((0, 26, 10, 1, 34)[g.integers(0, 5)])
    return cus, modes


def flat_planes(w, h, seed, chroma, amps=(0, 0, 0, 3, 10, 30)):
    """a source of flat areas with noise of one amplitude per 32x32 area (0 among them), so that large intra TUs keep coefficients at
    the low QPs only, or at none"""
    g = np.random.default_rng(seed)
    amp = np.kron(np.array(amps)[g.integers(0, len(amps), ((h + 31) // 32, (w + 31) // 32))], np.ones((32, 32), dtype=np.int64))[:h, :w]
    out = []
    for k in range(3 if chroma else 1):
        a = amp[::2, ::2] if k else amp
        out.append(np.clip(100 + 30 * k + np.rint((g.random(a.shape) * 2 - 1) * a), 0, 255).astype(np.uint8))
    return tuple(out) if chroma else (out[0], None, None)


def fixture_case(name, w, h, chroma, signhide, slice_is_intra, seed, intra_share, start_qp, lcu_qp):
    """-> (src, pred, cus, modes): a map of inter, intra and blank records; the prediction planes as motion compensation would leave
    them; a source that is the prediction plus noise inside the inter CUs and a picture of its own inside the intra CUs"""
    if name == "coarse":
        cus, modes = coarse_map(w, h, seed, intra_share)
    else:
        cus, _, modes = XC.make_map(w, h, seed, intra_share=intra_share, blank_share=0.08)
    pred = RC.smooth_planes(w, h, seed + 100, chroma)
    inter_src = RC.make_source(pred, cus, seed + 200, chroma)
    intra_src = flat_planes(w, h, seed + 300, chroma) if name == "coarse" else XC.make_planes(cus, seed + 300, chroma)[0]
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = tuple(np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) if (k == 0 or chroma) else None for k in range(3))
    return src, pred, cus, modes


def chain_case(w, h, seed, chroma=1):
    """-> (src, pred, cus, modes, lcu_qp) for the chain up to deblocking: every record is an inter CU with motion or an intra CU (the
    deblocking filter of the reference indexes the motion vectors of a record that is neither with mv_dir - 1 = -1, so a blank record
    is no input for it), and a QP per LCU drawn over the whole range"""
    cus, _, modes = XC.make_map(w, h, seed, intra_share=0.3, blank_share=0.0, bad_share=0.0, edge_cu=False)
    assert (cus["type"] != 0).all() and ((cus["type"] == IC.CU_INTRA) | (cus["mv_dir"] > 0)).all()
    pred = RC.smooth_planes(w, h, seed + 1, chroma)
    inter_src = RC.make_source(pred, cus, seed + 2, chroma)
    intra_src, _ = XC.make_planes(cus, seed + 3, chroma)
    m, mc, _ = XC.intra_mask(cus, w, h)
    src = tuple(np.where(mc if k else m, intra_src[k], inter_src[k]).astype(np.uint8) if (k == 0 or chroma) else None for k in range(3))
    lx, ly = lcu_grid(w, h)
    lcu_qp = np.random.default_rng(seed + 4).integers(0, 52, lx * ly).astype(np.int8)
    return src, pred, cus, modes, lcu_qp


def compose_chain(src, pred, cus, modes, lcu_qp, start_qp, chain_lcus=0, chroma=1, signhide=0, slice_is_intra=0, B=None, init=None, many=False):
    """inter residual -> intra reconstruction -> QP map.  -> (outputs of the inter stage, outputs after the intra stage, records with
    qp written, lcu_last_qp)"""
    mid = compose_inter(src, pred, cus, lcu_qp, chroma, signhide, slice_is_intra, B=B, init=init, many=many)
    full = compose_intra(src, mid["rec"], mid["cus"], modes, lcu_qp, chroma, signhide, slice_is_intra, B=B,
                         init=(mid["coeff"], mid["cbf_out"], mid["costs"]))
    mapped, last = set_cu_qps(full["cus"], full["cbf_out"], lcu_qp, start_qp, chain_lcus)
    return mid, full, mapped, last


def zero_outputs(w, h, chroma):
    """the outputs as the chain needs them: cbf_out cleared once by the caller; coefficients and costs poisoned"""
    coeff, _, cost = RC.initial_outputs(w, h, chroma)
    return coeff, np.zeros((h // 4, w // 4), np.uint8), cost


def coverage(inter_tus, intra_tus, lcu_qps, known=KNOWN_CASES):
    """what the populations fail to exercise -> list.  inter_tus: "tus" of compose_inter, intra_tus: of compose_intra (4:2:0 pictures),
    lcu_qps: every QP of every fixture array, known: the QP-map cases that the known answers contain"""
    missing = []
    for what, tus, qi in (("inter", inter_tus, 3), ("intra", intra_tus, 9)):
        for (p, sizes) in ((0, (4, 8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
            for n in sizes:
                for has in (0, 1):
                    if len({t[qi] for t in tus if t[0] == p and t[1] == n and t[2] == has}) < 2:
                        missing.append("%s plane %d size %d has_coeffs %d under two QPs" % (what, p, n, has))
    qs = sorted({int(v) for v in lcu_qps})
    for v in (0, 51):
        if v not in qs:
            missing.append("QP %d" % v)
    for r in range(6):
        if not any(v % 6 == r for v in qs):
            missing.append("a QP of residue %d mod 6" % r)
    if not any(30 <= v < 43 for v in qs):
        missing.append("a QP of 30 or more, where chroma departs from luma")
    if not any(v >= 43 for v in qs):
        missing.append("a QP at or above 43")
    for case in KNOWN_CASES:
        if case not in known:
            missing.append("QP map: " + case)
    return missing


def build_fixture(B=None):
    """numeric arrays only: per picture the source and prediction planes, the CU map (as bytes), the modes, the QP array and, over
    poisoned outputs (cbf_out cleared), what the chain leaves: planes, coefficients, cbf_out, costs (as uint32 [.., 6]), the records
    after the QP map for one chain and for row chains, and lcu_last_qp of both.  -> (dict, missing coverage)"""
    d, inter_tus, intra_tus, qps = {}, [], [], []
    for pic in FIXTURE_PICTURES:
        name, w, h, chroma, signhide, slice_is_intra, seed, share, start_qp, lcu_qp = pic
        src, pred, cus, modes = fixture_case(*pic)
        init = zero_outputs(w, h, chroma)
        mid, full, mapped, last = compose_chain(src, pred, cus, modes, lcu_qp, start_qp, 0, chroma, signhide, slice_is_intra, B=B, init=init)
        rows, last_rows = set_cu_qps(full["cus"], full["cbf_out"], lcu_qp, start_qp, lcu_grid(w, h)[0])
        if chroma:
            inter_tus += mid["tus"]
            intra_tus += full["tus"]
        qps += list(lcu_qp)
        for k, n in enumerate("yuv"):
            if src[k] is not None:
                d["%s_src_%s" % (name, n)], d["%s_pred_%s" % (name, n)] = src[k], pred[k]
                d["%s_rec_%s" % (name, n)], d["%s_coeff_%s" % (name, n)] = full["rec"][k], full["coeff"][k]
        as_bytes = lambda a: a.view(np.uint8).reshape(a.shape + (20,))
        d[name + "_cus"], d[name + "_modes"], d[name + "_lcu_qp"] = as_bytes(cus), modes, np.array(lcu_qp, np.int8)
        d[name + "_cus_out"] = as_bytes(full["cus"])
        d[name + "_cus_qp"], d[name + "_cus_qp_rows"] = as_bytes(mapped), as_bytes(rows)
        d[name + "_last"], d[name + "_last_rows"] = last, last_rows
        d[name + "_cbf_out"] = full["cbf_out"]
        d[name + "_costs"] = full["costs"].view(np.uint32).reshape(cus.shape + (6,))
        d[name + "_inter_tus"] = np.array(mid["tus"], dtype=np.int32).reshape(-1, 4)
        d[name + "_intra_tus"] = np.array(full["tus"], dtype=np.int32).reshape(-1, 10)
    return d, coverage(inter_tus, intra_tus, qps)


def load_fixture_case(z, name, chroma):
    """-> (src, pred, cus, modes, lcu_qp, want): want holds "full" (the outputs after the inter and the intra stage),
    "cus_qp" / "cus_qp_rows" and "last" / "last_rows\""""
    planes = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
    view = lambda a: np.ascontiguousarray(a).view(CU_INFO).reshape(a.shape[:2])
    costs = np.ascontiguousarray(z[name + "_costs"]).view(COST).reshape(z[name + "_costs"].shape[:2])
    full = {"rec": planes("rec"), "coeff": planes("coeff"), "cus": view(z[name + "_cus_out"]), "cbf_out": z[name + "_cbf_out"], "costs": costs}
    want = {"full": full, "cus_qp": view(z[name + "_cus_qp"]), "cus_qp_rows": view(z[name + "_cus_qp_rows"]),
            "last": z[name + "_last"], "last_rows": z[name + "_last_rows"]}
    return planes("src"), planes("pred"), view(z[name + "_cus"]), z[name + "_modes"], z[name + "_lcu_qp"], want


assert_outputs_equal = RC.assert_outputs_equal

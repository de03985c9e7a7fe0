"""Directed pictures for the deblocking filter: small pictures built class by class so that every decision the filter takes
(deblock_model.census_classes) is reached by at least COVERAGE_MIN segments in each direction, and so that every deliberate error
of the model (deblock_model.MUTANTS) changes the result on one of them.  TEST INFRASTRUCTURE.

A picture of the vertical set is a stack of bands.  A band is 128 pixels wide: four pairs of a 16-wide P region and a 16-wide Q region of
8 x 8 CUs; the band's 8-sample profile p3 .. q3 lies across the edge between P and Q on every line, p3 and q3 extended outwards, so that
the four target edges of a band are 8 (band of 8 lines) or 16 segments of one class.  What happens on the other edges -- between
two pairs, between two bands -- is not aimed at; the model filters and counts them as well.  Three pictures are built differently:
"amp" (32 x 32 CUs of every part mode over a staircase), "tiles" (a 2 x 2 tile grid over a staircase in both directions) and
"bs-b" (a B slice, one band per branch of the boundary strength).  The horizontal set is the transpose of every picture, its map
transposed with it (the part modes swap).

patterns.deblock_case and its seeds are not touched: random_cases() only calls it as test_gpu_parity.py::test_deblock_frame does."""
import functools

import numpy as np

import deblock_model as M
from patterns import CU_INFO, deblock_case, deblock_params

COVERAGE_MIN = 8
WIDTH = 128
FLAT = (100, 100, 100, 100, 110, 110, 110, 110)            # on for every bs > 0 at QP 22 and above; the result shows tc


def cu(type=2, cbf=0, mv_dir=1, mv0=(0, 0), mv1=(0, 0), ref0=0, ref1=0, qp=None):
    return dict(type=type, cbf_y=cbf, mv_dir=mv_dir if type == 2 else 0, mv=(mv0, mv1), mv_ref=(ref0, ref1), qp=qp)


INTRA, INTER, CODED, MOVED = cu(type=1), cu(), cu(cbf=1), cu(mv0=(8, 0))


def band(luma=FLAT, p=INTER, q=MOVED, u=(100, 100, 112, 112), v=(100, 100, 104, 104)):
    return dict(luma=luma, p=p, q=q, u=u, v=v)


def fill(cus, y0, y1, x0, x1, rec, qp, depth=3, part=0, tr_depth=3):
    blk = cus[y0 // 4:y1 // 4, x0 // 4:x1 // 4]
    blk["type"], blk["depth"], blk["part_size"], blk["tr_depth"] = rec["type"], depth, part, tr_depth
    blk["cbf_y"], blk["mv_dir"], blk["qp"] = rec["cbf_y"], rec["mv_dir"], qp if rec["qp"] is None else rec["qp"]
    blk["mv"], blk["mv_ref"] = rec["mv"], rec["mv_ref"]


def band_picture(name, prm, bands, band_h):
    """-> case: the bands from top to bottom, each band_h (8 or 16) lines high"""
    h = band_h * len(bands)
    y, u, v = np.zeros((h, WIDTH), np.uint8), np.zeros((h // 2, WIDTH // 2), np.uint8), np.zeros((h // 2, WIDTH // 2), np.uint8)
    cus = np.zeros((h // 4, WIDTH // 4), CU_INFO)
    qp = int(prm["qp"][0])
    for k, b in enumerate(bands):
        l, rows = b["luma"], slice(k * band_h, (k + 1) * band_h)
        y[rows] = np.tile([l[0]] * 12 + list(l) + [l[7]] * 12, 4)
        for plane, c in ((u, b["u"]), (v, b["v"])):
            plane[k * band_h // 2:(k + 1) * band_h // 2] = np.tile([c[0]] * 7 + [c[1], c[2]] + [c[3]] * 7, 4)
        for x0 in range(0, WIDTH, 32):
            fill(cus, rows.start, rows.stop, x0, x0 + 16, b["p"], qp)
            fill(cus, rows.start, rows.stop, x0 + 16, x0 + 32, b["q"], qp)
    chroma = bool(prm["chroma"][0])
    return dict(name=name, y=y, u=u if chroma else None, v=v if chroma else None, cus=cus, prm=prm, col_bd=None, row_bd=None)


def tables(beta, tc, qp, bs):
    """the picture parameters that give these beta and tc at this QP for edges of strength bs; asserts that they do"""
    for bo in range(-6, 7):
        for to in range(-6, 7):
            if 0 <= qp + 2 * bo <= 51 and 0 <= qp + 2 * (bs - 1) + 2 * to <= 53 and M.BETA_TABLE[qp + 2 * bo] == beta and \
                    M.TC_TABLE[qp + 2 * (bs - 1) + 2 * to] == tc:
                return dict(qp=qp, beta=bo, tc=to)
    raise AssertionError("no offsets give beta %d, tc %d at QP %d" % (beta, tc, qp))


# ---------------------------------------------------------------- the pictures of the vertical set
def strong_picture():
    """beta 50, tc 1, bs 1, 4:0:0: the strong filter and its thresholds.  tc52 = 3, beta >> 2 = 12, beta >> 3 = 6"""
    prm = deblock_params(chroma=0, **tables(50, 1, 32, 1))
    return band_picture("strong", prm, [
        band((105, 105, 105, 100, 102, 102, 102, 102)),          # p0 filters to 103, clipped at 100 + 2 tc
        band((95, 95, 95, 100, 98, 98, 98, 98)),                 # p0 filters to 97, clipped at 100 - 2 tc
        band((100, 100, 100, 100, 102, 102, 102, 102)),          # no sample clipped; |p0 - q0| = 2 = 5 tc >> 1
        band((103, 100, 100, 100, 101, 101, 101, 104)),          # |p3 - p0| + |q0 - q3| = 6 = beta >> 3: weak, delta 0
        band((100, 100, 100, 110, 110, 110, 125, 125)),          # dp + dq = 50 = beta: off
        band((100, 100, 100, 100, 118, 100, 100, 100)),          # weak, delta = 10 = 10 tc: the line is abandoned
        band((100, 140, 90, 130, 80, 150, 100, 60)),             # busy: off
    ], 8)


def weak_picture():
    """beta 64, tc 4, bs 1: the weak filter.  side threshold 12, tc52 = 10, tc >> 1 = 2"""
    prm = deblock_params(**tables(64, 4, 39, 1))
    return band_picture("weak", prm, [
        band((100, 100, 100, 100, 110, 110, 110, 110)),          # both second samples, delta = 4 = tc: not clipped
        band((100, 100, 100, 100, 116, 116, 116, 116)),          # delta 6, clipped at 4
        band((100, 100, 100, 100, 110, 110, 117, 117)),          # dq = 14: the second sample of P only
        band((93, 93, 100, 100, 110, 110, 110, 110)),            # dp = 14: the second sample of Q only
        band((93, 93, 100, 100, 110, 110, 117, 117)),            # neither
        band((102, 102, 100, 103, 115, 115, 115, 115)),          # the correction of p1 is 3, clipped at tc >> 1 = 2
        band((100, 106, 100, 100, 110, 110, 110, 110)),          # dp = 12 = side threshold: p1 stays
        band((247, 250, 250, 255, 255, 255, 255, 255)),          # |p3 - p0| = 8 = beta >> 3: weak; delta -1: q0 would be 256
        band((8, 5, 5, 0, 0, 0, 0, 0)),                          # delta 1: q0 would be -1
        band((255, 255, 255, 255, 255, 241, 227, 213)),          # delta 3: p0 would be 258, p1 256
        band((0, 0, 0, 0, 0, 14, 28, 42)),                       # delta -3: p0 would be -3, p1 -2
    ], 8)


def low_picture():
    """per-CU QPs of 10 to 17, no offsets: beta == 0 up to an edge QP of 15, and beta of 6 and 7 with tc == 0 at 16 and 17 (bs 1); the
    chroma of the intra CUs runs with tc == 0 as well"""
    prm = deblock_params(qp=14, per_cu_qp=1)
    at = lambda qp, rec: dict(rec, qp=qp)
    return band_picture("low", prm, [
        band(p=at(16, INTER), q=at(16, MOVED)), band(p=at(17, INTER), q=at(16, MOVED)), band(p=at(10, INTRA), q=at(11, INTER)),
        band(p=at(12, INTER), q=at(13, INTRA)), band(p=at(14, INTER), q=at(15, MOVED)), band(p=at(15, INTRA), q=at(15, INTRA)),
    ], 16)


def floor_picture():
    """QP 10 with both offsets at -6: both table indices are negative"""
    prm = deblock_params(qp=10, beta=-6, tc=-6)
    return band_picture("floor", prm, [band(), band(p=INTRA, q=INTER)], 8)


def high_picture():
    """QP 51 with both offsets at 6: both indices beyond their tables.  beta 64, tc 24"""
    prm = deblock_params(qp=51, beta=6, tc=6)
    return band_picture("high", prm, [
        band((100, 100, 100, 131, 131, 131, 131, 131)),          # dp + dq = 62: on below beta 64, off at beta[50] = 62
        band((100, 100, 100, 100, 152, 152, 152, 152)),          # delta 23: clipped at tc[52] = 22 only
        band(p=INTRA, q=INTRA),
    ], 8)


def bs_p_picture():
    """a P slice at QP 30: tc is 2 for bs 1 and 3 for bs 2, and FLAT's delta of 4 is clipped at it"""
    prm = deblock_params(qp=30)
    return band_picture("bs-p", prm, [
        band(p=INTRA, q=INTER), band(p=INTER, q=INTRA), band(p=INTRA, q=INTRA), band(p=INTER, q=CODED),
        band(p=INTER, q=cu(mv0=(4, 0))),                              # one list, vectors a whole pixel apart
        band(p=INTER, q=cu(mv_dir=2, mv1=(0, -8))),                    # L0 against L1
        band(p=INTER, q=cu(ref0=1)),                                  # the same vector into another picture
        band(p=cu(mv0=(3, 3)), q=cu(mv0=(0, 0))),                     # bs 0: less than a pixel apart
    ], 16)


B_REF_LX = ((0, 1, 2, 3), (0, 2, 3, 1))                   # L0 index i is picture i; L1 index 0, 1, 2 is picture 0, 2, 3


def bs_b_picture():
    """a B slice: one band per branch.  No coefficients anywhere, so that only references and vectors decide"""
    prm = deblock_params(qp=30, slice_is_b=1)
    prm["ref_LX"][0, 0, :4], prm["ref_LX"][0, 1, :4] = B_REF_LX
    bi = lambda mv0, mv1, ref0=0, ref1=1: cu(mv_dir=3, mv0=mv0, mv1=mv1, ref0=ref0, ref1=ref1)
    same = lambda mv0, mv1: bi(mv0, mv1, 0, 0)               # picture 0 on both lists
    return band_picture("bs-b", prm, [
        band(p=bi((0, 0), (20, 0)), q=bi((1, 0), (20, 3))),              # pictures (0, 2) on both sides, straight, near
        band(p=bi((0, 0), (20, 0)), q=bi((4, 0), (20, 0))),              # straight, far
        band(p=bi((0, 0), (20, 0)), q=bi((20, 0), (0, 0), 2, 0)),        # Q has (2, 0): cross-matched, near; the straight pairing is far
        band(p=bi((0, 0), (20, 0)), q=bi((20, 0), (9, 0), 2, 0)),        # cross-matched, far
        band(p=same((0, 0), (20, 0)), q=same((40, 0), (60, 0))),         # one picture on both lists: both pairings far
        band(p=same((0, 0), (20, 0)), q=same((20, 0), (0, 0))),          # straight far, cross near
        band(p=same((0, 0), (20, 0)), q=same((1, 0), (20, 0))),          # straight near, cross far
        band(p=same((0, 0), (0, 0)), q=same((1, 1), (0, 2))),            # both near
        band(p=bi((0, 0), (20, 0)), q=bi((0, 0), (20, 0), 0, 2)),        # (0, 2) against (0, 3)
        band(p=cu(mv_dir=1), q=bi((0, 0), (0, 0))),                      # uni-predicted against bi-predicted
        band(p=cu(mv_dir=1, mv1=(40, 40)), q=cu(mv_dir=2, mv0=(0, 0))),  # L0 -> picture 0 against L1 -> picture 0; P's unused vector is set
        band(p=cu(mv_dir=2, mv0=(-9, 40), ref1=1), q=cu(mv_dir=2, mv0=(30, 2), mv1=(2, 1), ref1=1)),   # straight, only unused vectors far
    ], 8)


def qp_picture():
    """per-CU QPs whose sums are odd where tc steps: the rounded average lands on the next tc"""
    prm = deblock_params(qp=30, per_cu_qp=1)
    at = lambda qp, rec: dict(rec, qp=qp)
    return band_picture("qp", prm, [band(p=at(a, INTER), q=at(b, MOVED)) for a, b in ((30, 31), (35, 34), (26, 27), (38, 37))], 16)


def chroma_picture():
    """intra CUs with per-CU QPs in all three parts of the chroma table"""
    prm = deblock_params(qp=36, per_cu_qp=1)
    at = lambda qp: dict(INTRA, qp=qp)
    return band_picture("chroma", prm, [
        band(p=at(20), q=at(20), u=(100, 100, 104, 104), v=(100, 100, 112, 112)),     # tc 1
        band(p=at(36), q=at(36), u=(100, 100, 112, 112), v=(112, 112, 100, 100)),     # QP 34 in chroma: tc 4, from the luma QP 5; delta 5
        band(p=at(48), q=at(48), u=(100, 100, 104, 104), v=(100, 100, 160, 160)),     # tc 11
        band(p=at(36), q=at(36), u=(255, 254, 255, 240), v=(240, 255, 254, 255)),     # delta 2: p0 / -2: q0 would be 256
        band(p=at(36), q=at(36), u=(0, 1, 0, 15), v=(15, 0, 1, 0)),                   # delta -2: p0 / 2: q0 would be -1
        band(p=at(10), q=at(10)),                                                     # tc 0
    ], 16)


def amp_picture():
    """128 x 64 of inter 32 x 32 CUs with one 32 x 32 TU each, every part mode, over a staircase with a step at every multiple of 8.
    The PUs of the first row of CUs and of the last two CUs differ by whole pixels; the PUs of the other CUs share their vector, and
    those CUs are coded: a PU edge with nothing to filter, whatever the cbf says"""
    prm = deblock_params(qp=30)
    y = np.tile((100 + 6 * (np.arange(WIDTH) // 8)).astype(np.uint8), (64, 1))
    u = np.tile((100 + 6 * (np.arange(WIDTH // 2) // 8)).astype(np.uint8), (32, 1))
    cus = np.zeros((16, WIDTH // 4), CU_INFO)
    sizes = (((4, 4),), ((4, 2), (4, 2)), ((2, 4), (2, 4)), ((2, 2),) * 4, ((4, 1), (4, 3)), ((4, 3), (4, 1)), ((1, 4), (3, 4)), ((3, 4), (1, 4)))
    for k, part in enumerate((6, 7, 2, 4, 6, 7, 1, 5)):
        x, y0, moving = 32 * (k % 4), 32 * (k // 4), k < 4 or k >= 6
        for i, (off, size) in enumerate(zip(M.PART_OFFSETS[part], sizes[part])):
            rec = cu(cbf=0 if moving else 1, mv0=(8 * i, 0) if moving else (2, 2))
            fill(cus, y0 + 8 * off[1], y0 + 8 * (off[1] + size[1]), x + 8 * off[0], x + 8 * (off[0] + size[0]), rec, 30, depth=1, part=part, tr_depth=1)
    return dict(name="amp", y=y, u=u, v=np.array(u[:, ::-1]), cus=cus, prm=prm, col_bd=None, row_bd=None)


def tiles_picture(name="tiles", tiled=True):
    """128 x 128 in 2 x 2 tiles of one LCU: a staircase in both directions, coded 8 x 8 CUs, every third one intra, so that every edge
    of the 8 x 8 grid is filtered -- but for those on the tile boundaries"""
    prm = deblock_params(qp=32)
    yy, xx = np.mgrid[0:WIDTH, 0:WIDTH]
    y = (60 + 5 * (xx // 8) + 5 * (yy // 8)).astype(np.uint8)
    u = np.ascontiguousarray(y[::2, ::2])
    cus = np.zeros((WIDTH // 4, WIDTH // 4), CU_INFO)
    for cy in range(0, WIDTH, 8):
        for cx in range(0, WIDTH, 8):
            fill(cus, cy, cy + 8, cx, cx + 8, INTRA if (cx // 8 + 2 * (cy // 8)) % 3 == 0 else CODED, 32)
    bd = [0, 1, 2] if tiled else None
    return dict(name=name, y=y, u=u, v=np.array(255 - u), cus=cus, prm=prm, col_bd=bd, row_bd=bd)


def transposed(case):
    cus = np.ascontiguousarray(case["cus"].T)
    cus["part_size"] = np.array(M.TRANSPOSED_PART, np.uint8)[cus["part_size"]]
    t = lambda p: None if p is None else np.ascontiguousarray(p.T)
    return dict(name=case["name"] + "^T", y=t(case["y"]), u=t(case["u"]), v=t(case["v"]), cus=cus, prm=case["prm"], col_bd=case["row_bd"],
                row_bd=case["col_bd"])


@functools.lru_cache(maxsize=None)
def _cases():
    vertical = [strong_picture(), weak_picture(), low_picture(), floor_picture(), high_picture(), bs_p_picture(), bs_b_picture(), qp_picture(),
                chroma_picture(), amp_picture(), tiles_picture(), tiles_picture("untiled", False)]
    out = vertical + [transposed(c) for c in vertical]
    for c in out:
        h, w = c["y"].shape
        assert w <= 192 and h <= 128 or w <= 128 and h <= 192, c["name"]
        assert (c["cus"]["type"] != 0).all() and ((c["cus"]["type"] == 1) | (c["cus"]["mv_dir"] != 0)).all()    # what the reference requires
        for a in (c["y"], c["u"], c["v"], c["cus"]):
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


def cases():
    """every directed picture: dicts of name, y, u, v (None for 4:0:0), cus, prm, col_bd, row_bd (None: not tiled).  Read-only"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def modelled(name, mutate=None):
    """-> ((y, u, v), census) of the model on the directed picture `name`; computed once"""
    c = {c["name"]: c for c in _cases()}[name]
    return M.deblock(c["y"], c["u"], c["v"], c["cus"], c["prm"], c["col_bd"], c["row_bd"], mutate)


# the pictures of test_gpu_parity.py::test_deblock_frame: its configurations, seeds and intra shares
RANDOM_CONFIGS = (dict(w=192, h=128, qp=34), dict(w=200, h=136, qp=38, beta=2, tc=-1), dict(w=128, h=64, qp=30, per_cu_qp=1),
                  dict(w=192, h=128, qp=36, slice_is_b=1), dict(w=136, h=72, qp=45, tc=3, per_cu_qp=1, slice_is_b=1),
                  dict(w=64, h=64, qp=22, beta=-3), dict(w=192, h=64, qp=40, chroma=0), dict(w=72, h=200, qp=51, beta=6, tc=6),
                  dict(w=8, h=8, qp=40), dict(w=640, h=360, qp=37, per_cu_qp=1, slice_is_b=1))


def random_cases(configs=RANDOM_CONFIGS, first_seed=300):
    """the random pictures of the GPU test (first_seed 300) or of the oracle's test against the reference (100), as cases"""
    out = []
    for k, cfg in enumerate(configs):
        cfg = dict(cfg)
        w, h = cfg.pop("w"), cfg.pop("h")
        prm = deblock_params(**cfg)
        for seed in range(3):
            y, u, v, cus = deblock_case(w, h, first_seed * k + seed, slice_is_b=int(prm["slice_is_b"][0]), qp=int(prm["qp"][0]),
                                        intra_share=(0.35, 0.0, 1.0)[seed])
            chroma = bool(prm["chroma"][0])
            out.append(dict(name="random %d/%d" % (k, seed), y=y, u=u if chroma else None, v=v if chroma else None, cus=cus, prm=prm,
                            col_bd=None, row_bd=None))
    return out


def coverage(cases_):
    """the merged census of the model over the cases"""
    total = M.collections.Counter()
    own = {id(c) for c in _cases()}
    for c in cases_:
        total += modelled(c["name"])[1] if id(c) in own else M.deblock(c["y"], c["u"], c["v"], c["cus"], c["prm"], c["col_bd"], c["row_bd"])[1]
    return total


def assert_coverage(census):
    """every class of the census in each direction -- and for chroma in each plane -- on COVERAGE_MIN segments at the least"""
    short = ["%s: %d" % (k, census.get(k, 0)) for k in M.census_classes() if census.get(k, 0) < COVERAGE_MIN]
    assert not short, "the pictures reach these classes on fewer than %d segments: %s" % (COVERAGE_MIN, ", ".join(short))


def first_difference(a, b):
    """-> "plane k (row, column): a != b" of the first pixel in which two results differ, or None"""
    for k, (p, q) in enumerate(zip(a, b)):
        if p is not None and (p != q).any():
            r, c = np.argwhere(p != q)[0]
            return "plane %d (%d, %d): %d != %d" % (k, r, c, p[r, c], q[r, c])
    return None


# ---------------------------------------------------------------- the fixture: inputs and the compiled reference's outputs
def expected(case, B):
    """what backend B (ref_lib or oracle_lib) makes of the case, tile by tile for the tiled picture"""
    import tile_chain_cases as TC
    if case["col_bd"] is not None:
        return TC.deblock((case["y"], case["u"], case["v"]), case["cus"], case["prm"], case["col_bd"], case["row_bd"], B)
    return B.deblock_frame(case["y"], case["u"], case["v"], case["cus"], case["prm"])


def build_fixture(B):
    d = {"names": np.array([c["name"] for c in cases()])}
    for c in cases():
        n = c["name"]
        want = expected(c, B)
        d[n + "/cus"], d[n + "/prm"] = np.ascontiguousarray(c["cus"]).view(np.uint8), np.ascontiguousarray(c["prm"]).view(np.uint8)
        d[n + "/tiles"] = np.array([c["col_bd"], c["row_bd"]] if c["col_bd"] is not None else [], np.int32)
        for k, p in enumerate("yuv"):
            if c[p] is not None:
                d["%s/%s" % (n, p)], d["%s/want_%s" % (n, p)] = c[p], want[k]
    return d


def load_fixture(z):
    """-> [(case, (y, u, v) expected)] as build_fixture stored them"""
    from patterns import DEBLOCK_PARAMS
    out = []
    for n in z["names"]:
        n = str(n)
        get = lambda key: z[n + "/" + key] if n + "/" + key in z.files else None
        tiles = z[n + "/tiles"]
        cus = z[n + "/cus"].view(CU_INFO)
        case = dict(name=n, y=get("y"), u=get("u"), v=get("v"), cus=cus.reshape(cus.shape[0], -1), prm=z[n + "/prm"].view(DEBLOCK_PARAMS),
                    col_bd=[int(b) for b in tiles[0]] if tiles.size else None, row_bd=[int(b) for b in tiles[1]] if tiles.size else None)
        out.append((case, (get("want_y"), get("want_u"), get("want_v"))))
    return out

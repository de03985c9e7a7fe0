"""Directed CU maps for the merge / AMVP candidate derivation: small pictures built class by class so that every decision of the
derivation (inter_cand_model.CLASSES) is reached by at least COVERAGE_MIN PUs, and so that every deliberate error of the model
(inter_cand_model.MUTANTS) changes the result of one of them.  TEST INFRASTRUCTURE.

Two kinds of picture.  A "tree" picture is a quadtree of CUs with every partition mode (patterns.inter_cu_map) under parameters
chosen for what they switch on or off: the slice type, the lists and the list that holds the searched picture, POC distances for each
clamp, tmvp, poc 1, an intra collocated picture, no references at all, an empty L0, tiles, no ref_cus.  A "lab" picture is a grid of
32 x 32 cells; a cell holds one 8 x 8 PU at (32 i, 32 j + 8) -- a place whose five neighbours all pass the coding-order tests -- and
its five neighbour SCUs, H and C3 are set one by one, everything else being intra: the combined pairs (each of the twelve table
positions), the duplicate tests, B2 at four candidates and the AMVP orders are spelled out there.

Every map is wider than its picture needs (cus_stride, col_stride).  The records outside the picture, the records of type 0 and
record 0 of every map carry wild vectors that name their place: a fetch from a wrong position shows.

patterns.inter_cand_case and its seeds are not touched: random_cases() only calls it as the existing tests do."""
import collections
import functools

import numpy as np

import inter_cand_model as M
from patterns import CU_INFO, INTER_CAND_CONFIGS, ME_PU, INTER_PARAMS, MERGE_CAND, inter_cand_case, inter_cu_map, inter_params

COVERAGE_MIN = 4
MAX_PUS = 256
EXTRA_CUS_STRIDE, EXTRA_COL_STRIDE = 3, 5


def wild(rows, stride, n_l0, n_l1, salt):
    """a map of inter records whose vectors name their column and row; directions and references within the lists"""
    m = np.zeros((rows, stride), CU_INFO)
    r, c = np.mgrid[0:rows, 0:stride]
    m["type"], m["depth"] = 2, 3
    m["mv_dir"] = 1 if not n_l1 else 2 if not n_l0 else 1 + c % 3
    m["mv"][..., 0, 0], m["mv"][..., 0, 1] = -(9000 + salt + c), 9000 + salt + r
    m["mv"][..., 1, 0], m["mv"][..., 1, 1] = 12000 + salt + r, -(12000 + salt + c)
    m["mv_ref"][..., 0], m["mv_ref"][..., 1] = c % max(n_l0, 1), (c // 2) % max(n_l1, 1)
    return m


def widen(inner, w, h, stride, n_l0, n_l1, salt, only=None):
    """the picture's records inside a wild map `stride` wide; records of type 0, and record 0, keep the wild motion"""
    rows = ((h + 63) // 64) * 16
    m = wild(rows, stride, n_l0, n_l1, salt)
    cut = np.array(inner[:(h + 3) // 4, :(w + 3) // 4])
    if only is not None:                                     # lists that exist: the directions of a picture with one list
        inter = cut["type"] == 2
        cut["mv_dir"][inter] = only
    keep = m[:cut.shape[0], :cut.shape[1]].copy()
    unset = cut["type"] == 0
    unset[0, 0] = True
    keep["type"] = 0
    cut[unset] = keep[unset]
    m[:cut.shape[0], :cut.shape[1]] = cut
    return m


def finish(name, p, cus, col, ref_cus, pus, seed):
    """-> the case: PUs that do not cover record 0, in shuffled order, MAX_PUS at the most, picture coordinates; maps read-only"""
    tx, ty = int(p["tile_x"][0]), int(p["tile_y"][0])
    pus = pus[(pus["x"] > 0) | (pus["y"] > 0)]
    g = np.random.default_rng(seed)
    pus = pus[g.permutation(len(pus))[:MAX_PUS]].copy()
    pus["x"] += tx
    pus["y"] += ty
    p = p.copy()
    p["cus_stride"], p["col_stride"] = cus.shape[1], col.shape[1]
    for a in (p, cus, col, ref_cus, pus):
        if a is not None:
            a.setflags(write=False)
    return (name, p, cus, col, ref_cus, pus)


# ---------------------------------------------------------------- tree pictures
# name, (w, h), inter_params keywords, list lengths of the current picture's CUs, of the collocated picture's CUs, options:
#   col_intra: the collocated picture is all intra; ref: "col" (the searched picture is the collocated one), "own" (a map of its own
#   with both lists) or None (no ref_cus); only: the one direction the current picture's CUs may have
TREES = [
    ("p-one-ref", (128, 72), dict(poc=8, ref_pocs=(7,), l0=(0,), col_ref_pocs=(6,), col_l0=(0,)), (1, 0), (1, 0), dict()),
    ("p-three-refs", (192, 136), dict(poc=12, ref_pocs=(11, 9, 4), l0=(0, 1, 2), ref_idx=1, col_ref_pocs=(9, 4, 2), col_l0=(0, 1, 2)), (3, 0), (3, 0),
     dict(ref="own")),
    ("p-far", (72, 128), dict(poc=200, ref_pocs=(199, 60, 2), l0=(0, 1, 2), ref_idx=2, col_ref_pocs=(60, 2), col_l0=(0, 1)), (3, 0), (2, 0),
     dict(ref="own")),
    ("p-no-tmvp", (128, 64), dict(poc=3, ref_pocs=(2,), l0=(0,), tmvp=0, col_ref_pocs=(1,), col_l0=(0,)), (1, 0), (1, 0), dict()),
    ("p-poc-1", (72, 72), dict(poc=1, ref_pocs=(0,), l0=(0,), col_ref_pocs=(-1,), col_l0=(0,)), (1, 0), (1, 0), dict()),
    ("p-col-intra", (128, 72), dict(poc=5, ref_pocs=(4,), l0=(0,), col_ref_pocs=(3,), col_l0=(0,)), (1, 0), (1, 0), dict(col_intra=True)),
    ("p-no-refs", (72, 64), dict(poc=6, ref_pocs=(), l0=(), col_ref_pocs=(3,), col_l0=(0,)), (1, 0), (1, 0), dict(ref=None)),
    ("p-tile-64-0", (128, 72), dict(poc=5, ref_pocs=(4, 2), l0=(0, 1), col_ref_pocs=(3, 1), col_l0=(0, 1), tile=(64, 0)), (2, 0), (2, 0), dict()),
    ("p-no-ref-cus", (128, 72), dict(poc=9, ref_pocs=(8, 6, 1), l0=(0, 1, 2), ref_idx=2, col_ref_pocs=(6, 4), col_l0=(0, 1)), (3, 0), (2, 0),
     dict(ref=None)),
    ("b-two-sided", (136, 72), dict(poc=4, ref_pocs=(0, 8), l0=(0, 1), l1=(1, 0), slice_is_b=1, ref_idx=1, col_ref_pocs=(8, 16), col_l0=(0,),
                                    col_l1=(1, 0)), (2, 2), (1, 2), dict(ref="own")),
    ("b-lowdelay", (104, 72), dict(poc=9, ref_pocs=(8, 7, 4), l0=(0, 1, 2), l1=(0, 1, 2), slice_is_b=1, ref_idx=0, col_ref_pocs=(7, 4), col_l0=(0, 1),
                                   col_l1=(0, 1)), (3, 3), (2, 2), dict()),
    ("b-hier", (136, 136), dict(poc=6, ref_pocs=(4, 8, 0, 16), l0=(0, 2, 1), l1=(1, 3, 0), slice_is_b=1, ref_idx=3, col_ref_pocs=(0, 8), col_l0=(0, 1),
                               col_l1=(1, 0)), (3, 3), (2, 2), dict(ref="own")),
    ("b-tile-64-64", (128, 72), dict(poc=4, ref_pocs=(2, 6), l0=(0, 1), l1=(1, 0), slice_is_b=1, ref_idx=0, col_ref_pocs=(0, 4), col_l0=(0, 1),
                                     col_l1=(1,), tile=(64, 64)), (2, 2), (2, 1), dict()),
    ("b-neither-list", (128, 72), dict(poc=5, ref_pocs=(4, 8, 2), l0=(0,), l1=(1,), slice_is_b=1, ref_idx=2, col_ref_pocs=(2, 6), col_l0=(0,),
                                       col_l1=(1,)), (1, 1), (1, 1), dict(ref="own")),
    ("b-l1-only", (128, 72), dict(poc=5, ref_pocs=(4, 8), l0=(0,), l1=(1,), slice_is_b=1, ref_idx=1, col_ref_pocs=(2, 6), col_l0=(0,), col_l1=(1,)),
     (1, 1), (1, 1), dict(ref="own")),
    # references 400 pictures after and 280 before; the collocated picture's lie 501 after and 289 before it
    ("b-far", (128, 72), dict(poc=300, ref_pocs=(299, 700, 20), l0=(0, 2), l1=(1, 0), slice_is_b=1, ref_idx=1, col_ref_pocs=(298, 800, 10),
                              col_l0=(0, 2), col_l1=(1, 0)), (2, 2), (2, 2), dict(ref="own")),
    ("b-far-lowdelay", (72, 72), dict(poc=300, ref_pocs=(299, 20), l0=(0, 1), l1=(1, 0), slice_is_b=1, ref_idx=1, col_ref_pocs=(800, 298),
                                      col_l0=(0, 1), col_l1=(1, 0)), (2, 2), (2, 2), dict()),
    ("b-empty-l0", (72, 72), dict(poc=8, ref_pocs=(7, 9), l0=(), l1=(0, 1), slice_is_b=1, ref_idx=0, col_ref_pocs=(6,), col_l0=(0,)), (0, 2), (1, 0),
     dict(only=2)),
    ("b-no-ref-cus", (72, 72), dict(poc=4, ref_pocs=(0, 8), l0=(0, 1), l1=(1,), slice_is_b=1, ref_idx=0, col_ref_pocs=(8,), col_l0=(0,), col_l1=(0,)),
     (2, 1), (1, 1), dict(ref=None)),
]


def tree_case(k, name, size, kw, cur_lists, col_lists, opt):
    w, h = size
    p = inter_params(w, h, **kw)
    tile = kw.get("tile", (0, 0))
    full_w, full_h = tile[0] + w, tile[1] + h
    cus, pus = inter_cu_map(w, h, 5000 + k, cur_lists[0], cur_lists[1], intra_share=0.15, unset_share=0.08)
    cus = widen(cus, w, h, ((w + 63) // 64) * 16 + EXTRA_CUS_STRIDE, cur_lists[0], cur_lists[1], 100 * k, opt.get("only"))
    col_stride = ((full_w + 63) // 64) * 16 + EXTRA_COL_STRIDE
    col, _ = inter_cu_map(full_w, full_h, 5100 + k, max(col_lists[0], 1), col_lists[1], intra_share=1.0 if opt.get("col_intra") else 0.25,
                          unset_share=0.0 if opt.get("col_intra") else 0.1)
    col = widen(col, full_w, full_h, col_stride, max(col_lists[0], 1), col_lists[1], 100 * k + 40)
    ref = opt.get("ref", "col")
    if ref == "own":
        ref_cus, _ = inter_cu_map(full_w, full_h, 5200 + k, 1, 1, intra_share=0.25, unset_share=0.1)
        ref_cus = widen(ref_cus, full_w, full_h, col_stride, 1, 1, 100 * k + 70)
    else:
        ref_cus = col if ref == "col" else None
    n_l0 = int(p["ref_LX_size"][0, 0])
    own_is_col = n_l0 > 0 and int(p["ref_idx"][0]) == int(p["ref_LX"][0, 0, 0])
    assert not (ref == "own" and own_is_col), name           # cu_arrays[ref_idx] IS the collocated array where the two are one picture
    return finish(name, p, cus, col, ref_cus, pus, 77 + k)


# ---------------------------------------------------------------- lab pictures
LAB_W, LAB_H = 192, 128
LAB_CELLS = [(cx, cy) for cy in (0, 32, 64, 96) for cx in (32, 64, 96, 128, 160)]


def rec(dir=1, mv0=(0, 0), mv1=(0, 0), ref0=0, ref1=0, type=2):
    return dict(type=type, mv_dir=dir, mv=(mv0, mv1), mv_ref=(ref0, ref1))


INTRA, UNSET = rec(type=1), rec(type=0)


def put(m, x, y, r, wild_map):
    c = m[y // 4, x // 4]
    if r["type"] == 0:                                       # not set: the wild motion is there
        m[y // 4, x // 4] = wild_map[y // 4, x // 4]
        c["type"] = 0
        return
    c["type"], c["mv_dir"], c["mv"], c["mv_ref"] = r["type"], r["mv_dir"] if r["type"] == 2 else 0, r["mv"], r["mv_ref"]
    if r["type"] != 2:
        c["mv"], c["mv_ref"] = 0, 0


def lab_case(name, kw, n_lists, col_lists, cells, seed):
    """cells: up to 20 dicts; keys a1, b1, b0, a0, b2 (records of the current picture), h, c3, centre (of the collocated one), pad;
    a key left out is an intra record (centre: a list-0 vector that names the cell).  The collocated picture is the searched one."""
    assert len(cells) <= len(LAB_CELLS), name
    p = inter_params(LAB_W, LAB_H, **kw)
    cus_stride, col_stride = 48 + EXTRA_CUS_STRIDE, 48 + EXTRA_COL_STRIDE
    cus, col = wild(32, cus_stride, n_lists[0], n_lists[1], 31), wild(32, col_stride, col_lists[0], col_lists[1], 57)
    wild_cus, wild_col = cus.copy(), col.copy()
    for m, wm in ((cus, wild_cus), (col, wild_col)):
        inside = m[:LAB_H // 4, :LAB_W // 4]
        inside["type"], inside["mv_dir"], inside["mv"], inside["mv_ref"] = 1, 0, 0, 0
        put(m, 0, 0, UNSET, wm)
    pus = np.zeros(len(cells), ME_PU)
    for k, (cell, (cx, cy)) in enumerate(zip(cells, LAB_CELLS)):
        x, y = cx, cy + 8
        pus[k]["x"], pus[k]["y"], pus[k]["width"], pus[k]["height"], pus[k]["pad"] = x, y, 8, 8, cell.get("pad", 0)
        cus[y // 4:y // 4 + 2, x // 4:x // 4 + 2]["type"] = 2
        cus[y // 4:y // 4 + 2, x // 4:x // 4 + 2]["mv_dir"] = 1
        for key, (nx, ny) in dict(a1=(x - 1, y + 7), a0=(x - 1, y + 8), b1=(x + 7, y - 1), b0=(x + 8, y - 1), b2=(x - 1, y - 1)).items():
            put(cus, nx, ny, cell.get(key, INTRA), wild_cus)
        put(col, x + 8, y + 8, cell.get("h", INTRA), wild_col)         # the top-left SCU of H's 16 x 16 block: (cx, cy + 16)
        assert ((x + 8) >> 4 << 4, (y + 8) >> 4 << 4) == (cx, cy + 16) and ((x + 4) >> 4 << 4, (y + 4) >> 4 << 4) == (cx, cy)
        put(col, cx, cy, cell.get("c3", INTRA), wild_col)
        put(col, x + 4, y + 4, cell.get("centre", rec(dir=1, mv0=(2 * k + 1, -k))), wild_col)   # the start vector's CU: neither H's nor C3's record
    return finish(name, p, cus, col, col, pus, seed)


def pair_cells(first, last):
    """for each table position k in first .. last, four cells whose merge list takes pair k and no earlier one: candidate i of the pair is
    the only one with a list-0 vector; the list-1 candidates before j in the table hold candidate i's picture and vector under a
    reference index of their own (all four indices of L1 name one picture), so they are no duplicates of each other but rejected pairs"""
    out = []
    for k in range(first, last + 1):
        i, j = M.PAIR_I[k], M.PAIR_J[k]
        n = 2 if k < 2 else 3 if k < 6 else 4
        for copy in range(4):
            m = (20 + 4 * k + copy, -3 - copy)
            cell = {}
            for c, key in enumerate(("a1", "b1", "b0", "a0")[:n]):
                if c == i:
                    cell[key] = rec(dir=1, mv0=m, mv1=(-700 - c, 700), ref0=0, ref1=3)
                elif c == j:
                    cell[key] = rec(dir=2, mv0=(800 + c, -800), mv1=(m[0] + 5, m[1]), ref1=c)
                else:
                    cell[key] = rec(dir=2, mv0=(800 + c, -800), mv1=m, ref1=c)
            out.append(cell)
    return out


def other_cells(mv):
    """the duplicate tests, B2 at four candidates, both orders of the combined pairs and the AMVP orders, on vectors around `mv`"""
    a, b, c, d = mv, (mv[0] + 9, mv[1]), (mv[0], mv[1] - 7), (mv[0] - 11, mv[1] + 2)
    l0 = lambda v, ref=0: rec(dir=1, mv0=v, mv1=(v[1] + 300, v[0] - 300), ref0=ref, ref1=2)
    l1 = lambda v, ref=0: rec(dir=2, mv0=(v[1] - 300, v[0] + 300), mv1=v, ref0=1, ref1=ref)
    bi = lambda v, u, r0=0, r1=0: rec(dir=3, mv0=v, mv1=u, ref0=r0, ref1=r1)
    return [
        dict(a1=l0(a), b1=l0(b), b0=l0(c), a0=l0(d), b2=l0((mv[0] + 40, mv[1]))),      # four candidates: B2 is not asked
        dict(a1=l0(a), b1=l0(a), b0=l0(a), a0=l0(a), b2=l0(a)),                        # every duplicate test answers yes
        dict(a1=l0(a), b1=l0(b), b0=l0(a), a0=l0(b), b2=l0(b)),                        # B0 equals A1, A0 equals B1: both kept; B2 equals B1
        dict(a1=l1(a), b1=l1(a, 1), b0=l1(a, 1), a0=l1(a, 2), b2=l1(a)),               # list 1 only: the reference index tells B1 and A0 from A1
        dict(a1=l0(a), b1=bi(a, b), b0=bi(a, c), a0=l1(b)),                            # one list against two
        dict(a1=bi(a, b), b1=bi(a, b), b0=bi(a, b, 1, 0), a0=bi(c, b)),                # bi-predictive duplicates but for one field
        dict(a1=l0(a), a0=l1(b), h=l0(c), c3=l0(d)),                                   # pair 0 and pair 1 want the other list each
        dict(a1=l1(a), b1=l0(a)),                                                      # pair 1: list 0 of B1 with list 1 of A1, one picture and vector
        dict(a1=l1(a), b1=l0(a, 1)),                                                   # the same vector in another picture
        dict(a0=l0(a), a1=l0(b, 1), b0=l0(c), b1=l0(d, 1), b2=l0(d)),                  # AMVP: A0 before A1, B0 before B1
        dict(a0=l1(a), a1=l1(b, 1), b0=l1(c), b1=l1(d, 1), b2=l1(d)),
        dict(b2=l0(a, 1), c3=l0(b)),                                                   # above only, another picture: scaled, and C3
        dict(b1=l0(a, 1), b2=l0(b), h=l1(c)),                                          # B1 scaled beside the unscaled B2
        dict(b0=l1(a, 1), h=l0(c)),
        dict(a1=l0(a, 1), b1=l0(b, 1), pad=2),                                         # B1 barred
        dict(a1=l0(a, 1), b1=l0(b, 1), pad=1),                                         # A1 barred: left of nothing, B1 scaled
        dict(a1=UNSET, b1=UNSET, b0=UNSET, a0=UNSET, b2=UNSET, h=UNSET, c3=UNSET),
        dict(a0=l0(a), b0=l0(a), h=l0(a)),                                             # two equal spatial candidates: the temporal one is asked
        dict(a1=l0(a, 1), a0=UNSET, b1=l0(a, 1), h=l0(b)),                             # scaled left; a scaled above one suppressed
        dict(a1=bi(a, b, 1, 1), b1=bi(c, d, 1, 0)),
    ]


LAB_B = dict(poc=8, ref_pocs=(7, 5), l0=(0, 1), l1=(0, 0, 0, 0), slice_is_b=1, ref_idx=0, tmvp=0, col_ref_pocs=(5,), col_l0=(0,), col_l1=(0,))
LAB_B2 = dict(poc=8, ref_pocs=(7, 5, 12), l0=(0, 1), l1=(0, 1, 2), slice_is_b=1, ref_idx=0, col_ref_pocs=(5, 9), col_l0=(0,), col_l1=(1, 0))
LAB_P = dict(poc=8, ref_pocs=(7, 5, 3), l0=(0, 1, 0), ref_idx=0, col_ref_pocs=(5,), col_l0=(0,), col_l1=(0,))


@functools.lru_cache(maxsize=None)
def _cases():
    out = [tree_case(k, *t) for k, t in enumerate(TREES)]
    out.append(lab_case("lab-pairs-0-4", LAB_B, (2, 4), (1, 1), pair_cells(0, 4), 1))
    out.append(lab_case("lab-pairs-5-9", LAB_B, (2, 4), (1, 1), pair_cells(5, 9), 2))
    out.append(lab_case("lab-pairs-10-11", LAB_B, (2, 4), (1, 1), pair_cells(10, 11) + other_cells((6, -2))[:12], 3))
    out.append(lab_case("lab-b", LAB_B2, (2, 3), (1, 2), other_cells((-14, 5)), 4))
    out.append(lab_case("lab-p", LAB_P, (3, 0), (1, 1), [{k: dict(v, mv_dir=1) if isinstance(v, dict) and v["type"] == 2 else v for k, v in c.items()}
                                                         for c in other_cells((3, 31))], 5))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    for (name, p, cus, col, ref_cus, pus) in out:
        w, h = int(p["pic_width"][0]), int(p["pic_height"][0])
        assert w <= 192 and h <= 136 and 0 < len(pus) <= MAX_PUS, name
        assert cus.shape[1] == int(p["cus_stride"][0]) > ((w + 63) // 64) * 16 and col.shape[1] == int(p["col_stride"][0]), name
        assert cus.shape[0] >= (h + 3) // 4 and col.shape[0] == ((int(p["in_height"][0]) + 63) // 64) * 16, name
        assert ref_cus is None or ref_cus.shape == col.shape, name
        defined_ground(name, p, cus, col)
    return tuple(out)


def defined_ground(name, p, cus, col):
    """what the reference needs to stay defined (patterns.inter_cand_case): no distance of zero to divide by, references within the lists"""
    p = p[0]
    n = int(p["num_refs"])
    pocs = [int(v) for v in p["ref_pocs"][:n]]
    assert int(p["poc"]) not in pocs, name
    sizes = [int(v) for v in p["ref_LX_size"]]
    for l in range(2):
        assert all(int(v) < n for v in p["ref_LX"][l][:sizes[l]]), name
        used = (cus["type"] == 2) & ((cus["mv_dir"] & (1 << l)) != 0)
        assert not used.any() or sizes[l] > 0 or n == 0, name
        assert (cus["mv_ref"][..., l][used] < max(sizes[l], 1)).all(), name
    assert ((cus["type"] != 2) | (cus["mv_dir"] != 0)).all() and ((col["type"] != 2) | (col["mv_dir"] != 0)).all(), name
    if n and sizes[0]:
        col_poc = pocs[int(p["ref_LX"][0][0])]
        for l in range(2):
            used = (col["type"] == 2) & ((col["mv_dir"] & (1 << l)) != 0)
            refs = np.unique(col["mv_ref"][..., l][used])
            assert all(int(p["col_ref_pocs"][int(p["col_ref_LX"][l][int(r)])]) != col_poc for r in refs), name


def cases():
    """every directed case: (name, params, cus, col, ref_cus, pus).  Read-only"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def modelled(name, mutant=None):
    """-> (pus_out, merge_out, census) of the model on the directed case `name`; computed once"""
    (_, p, cus, col, ref_cus, pus) = {c[0]: c for c in _cases()}[name]
    return M.derive(p, cus, col, ref_cus, pus, mutant)


def random_cases(which):
    """the random cases of test_gpu_parity.py::test_inter_candidates ("gpu test": seeds 1 .. 4 of every configuration) or of
    test_oracle_vs_ref.py::test_inter_candidates ("oracle test": seeds from 0 until a configuration has given 400 PUs), as cases"""
    out = []
    for c in INTER_CAND_CONFIGS:
        total, seed = 0, 1 if which == "gpu test" else 0
        while (seed <= 4) if which == "gpu test" else (total < 400):
            case = inter_cand_case(c[0], seed)
            for m in case:
                m.setflags(write=False)
            out.append(("%s/%d" % (c[0], seed),) + tuple(case))
            total += len(case[4])
            seed += 1
    return out


def coverage(cases_):
    """the merged census of the model over the cases"""
    total = collections.Counter()
    own = {id(c) for c in _cases()}
    for c in cases_:
        total += modelled(c[0])[2] if id(c) in own else M.derive(*c[1:])[2]
    return total


def assert_coverage(census):
    """every class of the census on COVERAGE_MIN PUs at the least, and none of the classes the reference cannot reach"""
    short = ["%s: %d" % (k, census.get(k, 0)) for k in M.census_classes() if census.get(k, 0) < COVERAGE_MIN]
    assert not short, "the cases reach these classes on fewer than %d PUs: %s" % (COVERAGE_MIN, ", ".join(short))
    assert not any(census.get(k, 0) for k in M.UNREACHABLE), "a class the reference's code cannot reach was counted"


def first_difference(a, b):
    """-> "PU k field: a != b" of the first record in which two results (pus_out, merge_out) differ, or None"""
    pa, pb = np.ascontiguousarray(a[0]).view(np.uint8).reshape(len(a[0]), -1), np.ascontiguousarray(b[0]).view(np.uint8).reshape(len(a[0]), -1)
    ma, mb = np.ascontiguousarray(a[1]).view(np.uint8).reshape(len(a[0]), -1), np.ascontiguousarray(b[1]).view(np.uint8).reshape(len(a[0]), -1)
    for i in np.flatnonzero((pa != pb).any(axis=1) | (ma != mb).any(axis=1)):
        if a[0][i] != b[0][i]:
            f = [n for n in a[0].dtype.names if not np.array_equal(a[0][i][n], b[0][i][n])][0]
            return "PU %d %s: %s != %s" % (i, f, a[0][i][f].tolist(), b[0][i][f].tolist())
        if (a[1][i] != b[1][i]).any():
            k = int(np.argwhere(a[1][i] != b[1][i])[0][0])
            return "PU %d merge[%d]: %s != %s" % (i, k, a[1][i][k], b[1][i][k])
    return None


# ---------------------------------------------------------------- the fixture: inputs and the compiled reference's outputs
def build_fixture(B):
    """B: ref_lib or oracle_lib.  Integer arrays and names only"""
    d = {"names": np.array([c[0] for c in cases()])}
    for (n, p, cus, col, ref_cus, pus) in cases():
        want_pus, want_merge = B.inter_candidates(p, cus, col, ref_cus, pus)
        d[n + "/prm"], d[n + "/pus"] = np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(pus).view(np.uint8).reshape(len(pus), 64)
        d[n + "/cus"], d[n + "/col"] = np.ascontiguousarray(cus).view(np.uint8), np.ascontiguousarray(col).view(np.uint8)
        # 0: no ref_cus, 1: the collocated picture's map, 2: a map of its own
        d[n + "/ref_kind"] = np.array([0 if ref_cus is None else 1 if ref_cus is col else 2], np.int32)
        if ref_cus is not None and ref_cus is not col:
            d[n + "/ref"] = np.ascontiguousarray(ref_cus).view(np.uint8)
        d[n + "/want_pus"] = np.ascontiguousarray(want_pus).view(np.uint8).reshape(len(pus), 64)
        d[n + "/want_merge"] = np.ascontiguousarray(want_merge).view(np.uint8).reshape(len(pus), 60)
    return d


def load_fixture(z):
    """-> [(case, want_pus as ME_PU [count], want_merge as MERGE_CAND [count, 5])] as build_fixture stored them"""
    out = []
    for n in z["names"]:
        n = str(n)
        maps = lambda key: np.ascontiguousarray(z[n + "/" + key]).view(CU_INFO)
        col = maps("col")
        kind = int(z[n + "/ref_kind"][0])
        case = (n, z[n + "/prm"].view(INTER_PARAMS), maps("cus"), col, None if kind == 0 else col if kind == 1 else maps("ref"),
                np.ascontiguousarray(z[n + "/pus"]).view(ME_PU).reshape(-1))
        out.append((case, np.ascontiguousarray(z[n + "/want_pus"]).view(ME_PU).reshape(-1),
                    np.ascontiguousarray(z[n + "/want_merge"]).view(MERGE_CAND).reshape(-1, 5)))
    return out

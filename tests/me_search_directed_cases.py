"""Directed cases for the motion search of one PU (search_pu_core, me_cost.h): 192 x 128 pictures and short PU lists that between them reach
every class of the census of tests/me_search_model.py, which the random inputs of the existing search tests do not.

What the random cases leave out (counted by the model over the inputs of test_gpu_parity.py::test_search_pu, all ME_CONFIGS, ::test_search_pu_mv_rdo,
::test_search_pu_flat_and_borders and ::test_search_pu_amp_smp_shapes, 9274 PUs, on which the model, the oracle and the compiled reference
agree; random_census() reproduces the count).  Of the 335 classes of the census they never reach 40:

    et:l2:equal-threshold                        the cost after a round exactly 0.95 of the cost before
    hex:steps:zero, hex:steps:one                max_steps 0 and 1 of the hexagon (the configurations have 2 and unlimited)
    dia:steps:zero, dia:steps:one                the same for the diamond, whose max_steps = 0 still runs one round
    full:lds:16:no-fit, full:lds:32:no-fit       an exhaustive-search window too large for the kernel's LDS in the two smaller size classes
    tie:et1:first-wins, tie:dia3:first-wins,     two candidates tie for the minimum of a group, below the incumbent, in the first
    tie:tz4:first-wins, tie:tz8:first-wins       early-termination round, the diamond's rounds and both tz patterns
    cost:merge:wrapped-equal-outside-int16       a vector outside int16 whose wrapped value is a merge candidate
    cost:golomb:2^k-1, 2^k, 2^k+1 for k = 9..15  |d| + 2 around the upper powers of two the fast path handles (21 classes)
    cost:golomb:fallback-x, fallback-y           |d| + 2 >= 2^16
    cost:lambda:0, cost:lambda:2^20              both edges of the entry's check on lambda_cost
    within:wpp:delay-none                        the WPP rule with neither SAO nor deblocking
    frac:gate:equal                              an integer cost equal to cost_to_beat
    shape:big-amp                                an AMP shape of the largest size class (64x16, 64x48, 16x64, 48x64)

They do reach a start group with no admissible vector and a negative numerator in the WPP rule's division, but with the bounds the
configurations use (down, right >= 0) truncation and floor admit the same vectors there: the mutant wpp-floor-division needs
max_ref_lcu_right = -1 to show.  And a class reached is not yet a decision tested: the result must depend on it, which is what the
mutants measure on the directed cases.

A case is (name, params ME_PARAMS [1], picture, reference, PUs ME_PU [n], CABAC snapshots ME_CABAC [m] or None, cost_to_beat uint32 [n]).  Most
cases steer the search with a cost bowl: a constant current block and a reference plane that grows with the distance from a chosen point, a
different slope on each side so that the sums over a block have one minimum; plateaus (the bowl quantised) give exact ties and costs equal to
the incumbent.  The cases named cover-* were found by a seeded random search over such pictures and parameters that kept a case when it added
a class (greedy cover) and are frozen here by their seed; the others are constructions, each described where it is built."""
import collections
import functools

import numpy as np

import me_search_model as M
from patterns import ME_CABAC, ME_PARAMS, ME_PU, ME_RESULT, me_cabac_states, me_frames, me_params, me_pus_in_tile, me_random_pus

W, H = 192, 128
MAX_INT = M.MAX_INT
U32 = M.U32
FIELDS = ("mv", "cost", "bitcost", "merged", "merge_idx", "mv_cand")
SHAPES = ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (24, 32), (32, 24), (16, 12), (12, 16),
          (8, 4), (4, 8), (16, 4), (4, 16), (32, 8), (8, 32), (64, 16), (16, 64), (64, 48), (48, 64))
TILES = ((64, 0, 128, 128), (0, 64, 192, 64), (64, 64, 64, 64), (0, 0, 128, 64))


# ---------------------------------------------------------------- pictures
def v_shape(n, at, down, up):
    """n values that fall with slope `down` to zero at `at` and rise with slope `up` after it"""
    i = np.arange(n)
    return np.where(i < at, (at - i) * down, (i - at) * up)


def bowl(x0, y0, slopes=(2, 3, 2, 3), base=0, step=1):
    """a cost bowl: base + a V in x around x0 + a V in y around y0, quantised to `step` (plateaus), clipped to a byte"""
    v = v_shape(W, x0, slopes[0], slopes[1])[None, :] + v_shape(H, y0, slopes[2], slopes[3])[:, None]
    return np.clip(base + v // step * step, 0, 255).astype(np.uint8)


def flat(v):
    return np.full((H, W), v, np.uint8)


def pu_list(rows):
    """rows of dict(x, y, w, h, cand=((x, y), (x, y)), extra=(x, y), merge=[(x, y, usable, same_ref)], snap=k)"""
    pus = np.zeros(len(rows), dtype=ME_PU)
    for i, r in enumerate(rows):
        pus[i]["x"], pus[i]["y"], pus[i]["width"], pus[i]["height"] = r["x"], r["y"], r["w"], r["h"]
        pus[i]["mv_cand"] = r.get("cand", ((0, 0), (0, 0)))
        pus[i]["extra_mv"] = r.get("extra", (0, 0))
        merge = r.get("merge", [])
        pus[i]["num_merge_cand"] = len(merge)
        for k, m in enumerate(merge):
            pus[i]["merge"][k]["mv"], pus[i]["merge"][k]["usable"], pus[i]["merge"][k]["same_ref"] = m[:2], m[2], m[3]
        pus[i]["reserved"] = r.get("snap", 0)
    return pus


def case(name, prm, pic, ref, pus, cabac=None, ctb=None):
    ctb = np.full(len(pus), MAX_INT, np.uint32) if ctb is None else np.asarray(ctb, dtype=np.uint32)
    assert pic.shape == ref.shape == (H, W) and len(ctb) == len(pus)
    return (name, prm, pic, ref, pus, cabac, ctb)


# ---------------------------------------------------------------- the seeded random search (greedy cover)
def random_steered_case(seed, name=None):
    """one case drawn from wide distributions of parameters, pictures (bowls, plateaus, flat planes, texture) and candidate lists"""
    g = np.random.default_rng(seed)
    pick = lambda seq: seq[int(g.integers(0, len(seq)))]
    alg = pick((0, 0, 0, 1, 1, 2, 2, 3))
    kw = dict(algorithm=alg, lambda_cost=pick((0, 1, 4, 20, 60, 500, 1 << 20)), early_termination=pick((0, 1, 1, 2, 2)),
              max_steps=pick((0xFFFFFFFF, 0xFFFFFFFF, 0, 1, 2, 3, 5)), fme_level=pick((0, 1, 2, 3, 4, 4)))
    if alg == 3:
        kw["search_range"] = pick((1, 2, 3, 5, 8))
    rule = pick(("none", "none", "none", "constraint", "constraint", "tile", "tile", "wpp", "wpp", "wpp-tile"))
    if rule in ("constraint", "tile", "wpp-tile"):
        kw["mv_constraint"] = pick((1, 2, 3, 4, 4)) if rule != "wpp-tile" else pick((0, 3, 4))
    if rule in ("tile", "wpp-tile"):
        kw["tile"] = pick(TILES)
    if rule in ("wpp", "wpp-tile"):
        kw.update(wpp_owf=1, ref_delay_px=pick((8, 10, 10, 0)), max_ref_lcu_down=pick((0, 1, 1, 2)), max_ref_lcu_right=pick((0, 1, 1, 2)))
    rdo = g.integers(0, 6) == 0
    if rdo:
        refs_before = pick((1, 2, 3, 5))
        kw.update(mv_rdo=1, refs_before=refs_before, ref_idx=int(g.integers(0, refs_before)))
    prm = me_params(**kw)
    # the PUs
    n = 4
    rows = []
    scale = pick((6, 40, 40, 300))
    mv = lambda: tuple(int(v) for v in g.integers(-scale, scale + 1, 2))
    tile = kw.get("tile", (0, 0, W, H))
    for i in range(n):
        w, h = pick(SHAPES)
        w, h = min(w, tile[2]), min(h, tile[3])
        place = pick(("any", "any", "left", "right", "top", "bottom", "corner"))
        x = int(g.integers(0, (tile[2] - w) // 4 + 1)) * 4
        y = int(g.integers(0, (tile[3] - h) // 4 + 1)) * 4
        if place in ("left", "corner"):
            x = 0
        if place == "right":
            x = tile[2] - w
        if place in ("top", "corner"):
            y = 0
        if place == "bottom":
            y = tile[3] - h
        r = dict(x=tile[0] + x, y=tile[1] + y, w=w, h=h, snap=i % 3)
        c0 = mv()
        r["cand"] = (c0, c0 if g.integers(0, 4) == 0 else mv())
        style = int(g.integers(0, 5))
        r["extra"] = (0, 0) if style == 0 else mv() if style < 3 else tuple(int(v) * 4 for v in g.integers(-70, 71, 2))
        merge = []
        for k in range(int(g.integers(0, 6))):
            kind = int(g.integers(0, 8))
            m = mv() if kind < 3 else r["cand"][kind % 2] if kind < 5 else r["extra"] if kind == 5 else tuple(int(v) for v in g.integers(-3, 4, 2)) \
                if kind == 6 else (merge[-1][:2] if merge else (0, 0))
            merge.append((m[0], m[1], int(g.integers(0, 4) != 0), int(g.integers(0, 3) != 0)))
        r["merge"] = merge
        rows.append(r)
    pus = pu_list(rows)
    # the pictures: a bowl whose centre lies near where the first PU would have to go
    kind = pick(("bowl", "bowl", "bowl", "plateau", "plateau", "texture", "flat"))
    if kind in ("bowl", "plateau"):
        far = pick((6, 20, 20, 70))
        cx = rows[0]["x"] + rows[0]["w"] // 2 + int(g.integers(-far, far + 1))
        cy = rows[0]["y"] + rows[0]["h"] // 2 + int(g.integers(-far, far + 1))
        slopes = tuple(int(v) for v in g.integers(1, 4, 4))
        base = int(g.integers(0, 30))
        ref = bowl(cx, cy, slopes, base, pick((4, 8, 16)) if kind == "plateau" else 1)
        pic = flat(base) if g.integers(0, 3) else bowl(cx + int(g.integers(-9, 10)), cy + int(g.integers(-9, 10)), slopes, base)
    elif kind == "texture":
        pic, ref = me_frames(W, H, 5000 + seed, tuple(int(v) for v in g.integers(-12, 13, 2)))
    else:
        pic, ref = flat(77), flat(77 + int(g.integers(0, 2)))
    cabac = me_cabac_states(3, 100 + seed) if rdo else None
    ctb = None
    if g.integers(0, 5) == 0:
        ctb = g.choice(np.array([MAX_INT, 1, 400, 3000, 20000], dtype=np.uint32), n)
    return case(name or "cover-%d" % seed, prm, pic, ref, pus, cabac, ctb)


def _seed_census(seed):
    c = random_steered_case(seed)
    return seed, set(M.search_pu_batch(c[2], c[3], c[4], c[1], c[5], c[6])[1])


def greedy_cover(seeds, have, workers=8):
    """how COVER was found: the seeds, in order, whose case reaches a class that neither `have` nor an earlier seed reaches -> [(seed, a class it added)]"""
    import multiprocessing
    have, kept = set(have), []
    with multiprocessing.Pool(workers) as pool:
        for seed, reached in pool.imap(_seed_census, seeds, chunksize=8):
            new = sorted(reached - have - set(M.UNREACHABLE))
            if new:
                kept.append((seed, new[0].replace(":", "-")))
                have |= reached
    return kept


# the seeds the greedy cover kept, with a class each added when it was found
COVER = (
    (0, "tie-et1-equals-incumbent"), (1, "et-r2-after0-none"), (2, "cost-merge-usable-not-same-ref"), (3, "frac-refused-would-have-won"),
    (4, "cost-lambda-two-to-20"), (5, "within-c4-refused-bottom"), (6, "dia-steps-zero"), (7, "full-merge0-zero"), (10, "et-r2-after0-p2"),
    (12, "start-winner-merge2"), (13, "cost-merged-idx2"), (14, "et-r2-after3-p0"), (15, "full-jump-merge3"), (16, "frac-qpel-win5"),
    (18, "full-merge1-zero"), (19, "dia-first-win3"), (21, "hex-from8"), (22, "frac-qpel-win3"), (24, "frac-hpel-win6"), (26, "et-r2-after0-p0"),
    (27, "et-r2-after1-p2"), (29, "full-jump-merge2"), (30, "hex-steps-one"), (31, "dia-first-centre"), (37, "et-r2-after1-none"),
    (38, "et-r2-after2-none"), (39, "full-merge4-unusable"), (40, "dia-loop-win3"), (46, "et-r2-after2-p0"), (47, "hex-small-win2"),
    (49, "within-c3-pass"), (53, "within-c3-refused-bottom"), (55, "cost-merged-idx4"), (57, "hex-steps-exactly-enough"), (58, "dia-steps-ran-out"),
    (79, "start-winner-merge3"), (80, "frac-qpel-win6"), (81, "cost-merged-idx3"), (83, "et-r2-after1-p0"), (92, "tie-dia5-first-wins"),
    (122, "tz-run2-to-end"), (125, "dia-steps-one"), (180, "hex-small-win7"), (284, "hex-small-win8"), (286, "hex-small-win5"),
    (350, "et-r2-after3-p2"), (551, "hex-from8-decides-the-path"),
)


# ---------------------------------------------------------------- constructions
def integer_cost_of(pic, ref, pu, prm):
    """the cost the integer search ends with (the value the gate of the fractional stage compares)"""
    p = prm.copy()
    p["fme_level"] = 0
    s = M._Search(pic, ref, pu, np.ascontiguousarray(p).reshape(-1)[0], None, None, None, None, None)
    {0: s.hexagon, 1: s.diamond, 2: s.tz, 3: s.full}[s.alg]()
    return s.best_cost


def _golomb_edges():
    """|d| + 2 at 2^k - 1, 2^k and 2^k + 1 for k = 2 .. 15: the two AMVP candidates carry four such distances per PU from the zero vector,
    on flat pictures, where the bits alone decide; every sign"""
    values = [(1 << k) + o - 2 for k in range(2, 16) for o in (-1, 0, 1)]
    values += [values[-1], values[0]]
    rows = []
    for i in range(0, len(values), 4):
        a, b, c, d = values[i:i + 4]
        s = 1 if (i // 4) % 2 else -1
        rows.append(dict(x=8 * (i // 4) + 16, y=32 + 8 * ((i // 4) % 3), w=8, h=8, cand=((s * a, -s * b), (-s * c, s * d)), extra=(4 * s, -4 * s)))
    return case("golomb-power-edges", me_params(lambda_cost=3, early_termination=0, fme_level=0), flat(90), flat(90), pu_list(rows))


def _outside_int16():
    """start vectors at +32767 quarter-pel: the block lies wholly outside the picture and the hexagon's first ring moves it to 8192 (8193)
    pixels, outside int16 in quarter-pel.  The picture's last column (row) is a V that makes exactly that point the best, max_steps = 0
    keeps it.  The AMVP candidates at -32768 put |d| + 2 past 2^16 in x (in y), and a merge candidate sits at the value the vector wraps to"""
    ref = flat(0)
    ref[:, W - 1] = np.clip(100 + v_shape(H, 66, 5, 7), 0, 255)      # 8 rows from 62 (PU at 64, dy = -2) cost least
    ref[H - 1, :] = np.clip(100 + v_shape(W, 67, 5, 7), 0, 255)      # 8 columns from 63 (PU at 64, dx = -1) cost least
    ref[H - 1, W - 1] = 255
    rows = [dict(x=0, y=64, w=8, h=8, cand=((-32768, 0), (-32768, -8)), extra=(32767, 0), merge=[(7, 7, 1, 1), (-32768, -8, 1, 1)]),
            dict(x=64, y=0, w=8, h=8, cand=((0, -32768), (-4, -32768)), extra=(0, 32767), merge=[(-4, -32764, 1, 1)]),
            dict(x=0, y=64, w=8, h=8, cand=((-32768, 0), (-32768, -8)), extra=(32767, 0), merge=[(-32768, -8, 1, 0), (-32768, -8, 0, 1)])]
    return case("start-outside-int16", me_params(lambda_cost=1, early_termination=0, fme_level=0, max_steps=0), flat(100), ref, pu_list(rows))


def _none_admissible():
    """wpp_owf with max_ref_lcu_down = 0: for a PU whose bottom row plus the margin reaches the next LCU row even the zero vector is refused,
    and every point of the hexagon, the diamond and the two early-termination rounds with it: best_cost stays 0xffffffff"""
    rows = [dict(x=16 * i, y=48, w=8, h=8, cand=((3, 1), (-2, 0)), extra=(4, 0), merge=[(8, 4, 1, 1)]) for i in range(2)]
    out = []
    for k, kw in enumerate((dict(algorithm=0, early_termination=0), dict(algorithm=1, early_termination=1), dict(algorithm=0, early_termination=2, fme_level=2))):
        prm = me_params(wpp_owf=1, ref_delay_px=10, max_ref_lcu_down=0, max_ref_lcu_right=1, lambda_cost=5, **kw)
        out.append(case("no-admissible-start-%d" % k, prm, flat(50), bowl(30, 60), pu_list(rows)))
    return out


def _wpp_negative_numerator():
    """max_ref_lcu_right = -1: only vectors whose LCU difference in x is -1 are admitted.  C's division truncates, so from the first LCU
    column that takes a numerator of -256 or less (80 pixels to the left); a floor would admit every negative numerator (17 pixels)"""
    prm = me_params(wpp_owf=1, ref_delay_px=8, max_ref_lcu_down=0, max_ref_lcu_right=-1, lambda_cost=2, early_termination=0, fme_level=0)
    rows = [dict(x=0, y=8, w=8, h=8, extra=(-30 * 4, 0)), dict(x=0, y=24, w=8, h=8, extra=(-90 * 4, 0)),
            dict(x=0, y=8, w=8, h=8, extra=(-81 * 4, 4), merge=[(-79 * 4, 0, 1, 1)]), dict(x=64, y=8, w=8, h=8, extra=(-30 * 4, 0))]
    return case("wpp-negative-numerator", prm, flat(10), bowl(-40, 12), pu_list(rows))


def _threshold_equal():
    """early_termination = 2 with the cost after the first round exactly 0.95 of the cost before: 4000 -> 3800.  The search ends there
    although two pixels to the left cost far less"""
    f = np.full(W, 255, np.int64)
    px = 40
    f[px:px + 7], f[px + 7], f[px - 1], f[px - 2], f[px - 3:px - 10:-1] = 62, 66, 41, 0, 0
    ref = np.broadcast_to(f.astype(np.uint8)[None, :], (H, W)).copy()
    assert 4000 * 0.95 == 3800
    rows = [dict(x=px, y=16, w=8, h=8), dict(x=px, y=48, w=8, h=8, extra=(4, 8))]
    out = [case("et2-cost-at-threshold-%s" % n, me_params(lambda_cost=0, early_termination=2, fme_level=0, algorithm=a), flat(0), ref, pu_list(rows))
           for n, a in (("hex", 0), ("dia", 1), ("tz", 2))]
    return out


def _gate():
    """cost_to_beat equal to the integer search's cost, one below and one above it, for each algorithm and fme_level 1 .. 4"""
    out = []
    pic, ref = me_frames(W, H, 71, (5, -3))
    for k, (alg, fme) in enumerate(((0, 4), (1, 2), (2, 3), (3, 1))):
        prm = me_params(algorithm=alg, fme_level=fme, lambda_cost=12, search_range=4)
        base = pu_list([dict(x=40 + 8 * k, y=24 + 16 * k, w=w, h=h, cand=((-18, 10), (-22, 14)), extra=(-20, 12)) for w, h in ((8, 8), (16, 16), (32, 32))])
        pus = np.repeat(base, 3)
        ctb = []
        for i in range(len(base)):
            c = integer_cost_of(pic, ref, base[i], prm)
            ctb += [c, c - 1, c + 1]
        out.append(case("gate-%d" % k, prm, pic, ref, pus, None, ctb))
    return out


def _full_windows():
    """the exhaustive search: windows that fit the kernel's LDS and windows that do not in the two smaller size classes, the largest PU at the
    largest range, windows of merge candidates that overlap each other, the zero window and the window of an unusable earlier candidate"""
    out = []
    ref = bowl(100, 70, (2, 3, 3, 2), 5)
    for name, w, h, rng in (("16-fits", 8, 8, 8), ("16-no-fit", 16, 16, 32), ("32-fits", 32, 32, 8), ("32-no-fit", 24, 32, 48), ("64-r64", 64, 64, 64)):
        assert M.window_fits(w, h, rng) == (not name.endswith("no-fit"))
        rows = [dict(x=64, y=32, w=w, h=h, cand=((40, -8), (60, 20)), extra=(0, 0) if rng == 64 else (rng * 4 + 8, -rng * 4))]
        out.append(case("full-lds-" + name, me_params(algorithm=3, search_range=rng, lambda_cost=6, fme_level=2 if rng < 64 else 0), flat(5), ref, pu_list(rows)))
    # overlapping windows at range 3: merge 0 unusable (its window must not count), 1 overlaps the zero window, 2 overlaps 1, 3 rounds to zero, 4 far away
    merges = [(20, 8, 0, 1), (16, 8, 1, 1), (28, 20, 1, 0), (3, 2, 1, 1), (60, -40, 1, 1)]
    rows = [dict(x=80 + 16 * i, y=48, w=8, h=8, cand=((24, 12), (24, 12)), extra=e, merge=merges[:5 - i]) for i, e in enumerate(((44, 16), (16, 8), (-20, 30)))]
    for k, (cx, cy) in enumerate(((95, 57), (112, 50), (99, 54))):
        out.append(case("full-overlapping-windows-%d" % k, me_params(algorithm=3, search_range=3, lambda_cost=0 if k else 9, fme_level=k, mv_constraint=0),
                        flat(5), bowl(cx, cy, (3, 2, 2, 3), 5), pu_list(rows)))
    # the best position lies (a) inside the window of the unusable merge 0 and of merge 1, outside the zero window: it must be searched;
    # (b) one column to the right of the zero window, inside merge 0's: the jump past the zero window must land on it.  An 8-wide block
    # costs least where it starts 4 before the bowl's centre (slopes 2 and 3)
    prm = me_params(algorithm=3, search_range=3, lambda_cost=0, fme_level=0)
    out.append(case("full-best-in-unusable-earlier-window", prm, flat(0), bowl(80 + 6 + 4, 48 + 3 + 4),
                    pu_list([dict(x=80, y=48, w=8, h=8, merge=[(20, 8, 0, 1), (16, 8, 1, 1)])])))
    out.append(case("full-best-right-after-the-jump", prm, flat(0), bowl(80 + 4 + 4, 48 + 1 + 4), pu_list([dict(x=80, y=48, w=8, h=8, merge=[(16, 8, 1, 1)])])))
    prm = me_params(algorithm=3, search_range=4, lambda_cost=3, fme_level=0, mv_constraint=1)
    rows = [dict(x=0, y=0, w=16, h=8, merge=[(12, 8, 1, 1), (-8, 12, 1, 1)], extra=(8, -8)), dict(x=W - 8, y=H - 16, w=8, h=16, merge=[(-12, -8, 1, 1)], extra=(12, 4))]
    out.append(case("full-within-false-in-window", prm, flat(5), bowl(4, 3, (2, 3, 3, 2), 5), pu_list(rows)))
    return out


def _shapes_and_borders():
    """every size class's fixed and generic shapes at each border, pulled outside the picture by a bowl whose centre lies beyond it, and start
    vectors that put the block wholly outside"""
    out = []
    shapes = ((8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (12, 16), (24, 32), (16, 12), (64, 16), (48, 64), (16, 8), (32, 16))
    for k, (cx, cy, side) in enumerate(((-30, 60, "left"), (W + 30, 60, "right"), (90, -30, "top"), (90, H + 30, "bottom"))):
        rows = []
        for i, (w, h) in enumerate(shapes):
            x = 0 if side == "left" else W - w if side == "right" else (8 * i) % (W - w + 1) // 4 * 4
            y = 0 if side == "top" else H - h if side == "bottom" else (12 * i) % (H - h + 1) // 4 * 4
            far = {"left": (-4 * (w + 20), 0), "right": (4 * (w + 20), 8), "top": (4, -4 * (h + 20)), "bottom": (0, 4 * (h + 20))}[side]
            rows.append(dict(x=x, y=y, w=w, h=h, cand=((far[0] // 2, far[1] // 2), (0, 0)), extra=far if i % 2 else (0, 0)))
        prm = me_params(algorithm=(0, 1, 2, 0)[k], lambda_cost=2, early_termination=k % 2, fme_level=(4, 2, 3, 1)[k])
        out.append(case("border-%s" % side, prm, flat(20), bowl(cx, cy, (1, 1, 1, 1), 20), pu_list(rows)))
    return out


def _tz_distances():
    """tz: a bowl whose centre lies 1, 2, 4 .. 64 pixels from the start, so that each distance of the first grid run is the last to improve,
    from the zero vector (no second run) and from a start vector (second run from (0, 0)); the far ones leave the picture on every side"""
    out = []
    for k, (dx, dy) in enumerate(((1, 0), (0, -2), (-4, 0), (0, 8), (16, 0), (0, -32), (-64, 0), (0, 64), (64, 0), (0, -64), (40, 24), (-90, 0))):
        px, py = (88, 56) if max(abs(dx), abs(dy)) < 64 else (24 if dx > 0 else W - 32 if dx < 0 else 88, 8 if dy > 0 else H - 16 if dy < 0 else 56)
        rows = [dict(x=px, y=py, w=8, h=8, cand=((4 * dx, 4 * dy), (0, 0))),
                dict(x=px, y=py, w=8, h=8, cand=((0, 0), (0, 0)), extra=(12, -8), merge=[(4 * dx, 4 * dy, 0, 1)])]
        prm = me_params(algorithm=2, lambda_cost=0 if k % 2 else 1, early_termination=0, fme_level=k % 3)
        out.append(case("tz-bowl-at-%d-%d" % (dx, dy), prm, flat(0), bowl(px + dx + 4, py + dy + 4, (2, 3, 2, 3)), pu_list(rows)))
    # two basins: a shallow bowl near (10, 5) and a block of zeros exactly 64 pixels to the right of the PU, which only a pattern point at
    # (64, 0) finds.  From the zero vector the first grid run reaches it at distance 64; from a start vector near the bowl nothing does: the
    # second run from (0, 0) stops at 48 and no point of a star around the bowl's minimum comes within 8 pixels of it
    px, py = 40, 56
    ref = bowl(px + 10 + 4, py + 5 + 4, (1, 1, 1, 1), 60)
    ref[py:py + 8, px + 64:px + 72] = 0
    rows = [dict(x=px, y=py, w=8, h=8), dict(x=px, y=py, w=8, h=8, extra=(48, 24))]
    out.append(case("tz-two-basins-64-from-zero", me_params(algorithm=2, lambda_cost=0, early_termination=0, fme_level=0), flat(0), ref, pu_list(rows)))
    # stepping stones: 8 x 8 squares of falling value in a plane of 255, at the start vector and at the points of the second grid run (from
    # (0, 0)) of distance 4, 8, 16 and 32, so that this run fails only twice and goes on to its last distance.  A square of zeros at (64, 0)
    # waits for a run that went on to 64: the reference's stops at 48
    px, py = 64, 48
    ref = flat(255)
    for (dx, dy), v in (((-16, -12), 200), ((0, -4), 180), ((8, 0), 160), ((0, 16), 140), ((16, 16), 120), ((64, 0), 0)):
        ref[py + dy:py + dy + 8, px + dx:px + dx + 8] = v
    rows = [dict(x=px, y=py, w=8, h=8, extra=(-64, -48))]
    out.append(case("tz-stepping-stones-second-run-ends-at-48", me_params(algorithm=2, lambda_cost=0, early_termination=0, fme_level=0), flat(0), ref, pu_list(rows)))
    return out


def _rdo():
    """--mv-rdo: merged vectors at every index, refs_before 1, 2 and more with ref_idx 0 and above, snapshots with either MPS in every context"""
    out = []
    pic, ref = me_frames(W, H, 72, (-2, 3))
    for k, (refs_before, ref_idx, alg) in enumerate(((1, 0, 0), (2, 0, 1), (2, 1, 0), (4, 0, 2), (4, 2, 0), (5, 4, 3))):
        cab = me_cabac_states(4, 40 + k)
        cab["ctx"][0, :7] = (cab["ctx"][0, :7] & 0xFE) | (k & 1)                 # one snapshot with the same MPS in every context ...
        cab["ctx"][1, :7] = (cab["ctx"][1, :7] & 0xFE) | (~k & 1)                # ... and one with the other
        rows = []
        for i in range(6):
            m = [(9 + i, -11, 1, 1), (8, -12, 1, 1), (8, -12, 1, 1), (4 * i, 4, 1, i % 2), (10, -14, 1, 1)]
            m[i % 5] = (8, -12 + (i // 5), 1, 1)
            rows.append(dict(x=16 + 24 * i, y=40 + 4 * (i % 3), w=(8, 16, 32, 8, 16, 12)[i], h=(8, 16, 32, 16, 8, 16)[i],
                             cand=((8, -12), (8, -12)) if i == 5 else ((6 + i, -10), (12, -16 + i)), extra=(8, -12), merge=m[:5 - (i == 4)], snap=i % 4))
        prm = me_params(mv_rdo=1, refs_before=refs_before, ref_idx=ref_idx, algorithm=alg, search_range=3, lambda_cost=7 + 9 * k, fme_level=(4, 0, 2, 3, 1, 4)[k])
        out.append(case("mv-rdo-%d" % k, prm, pic, ref, pu_list(rows), cab))
    return out


CONSTRUCTIONS = (_golomb_edges, _outside_int16, _none_admissible, _wpp_negative_numerator, _threshold_equal, _gate, _full_windows, _shapes_and_borders,
                 _tz_distances, _rdo)


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for build in CONSTRUCTIONS:
        got = build()
        out += got if isinstance(got, list) else [got]
    out += [random_steered_case(seed, "cover-%d-%s" % (seed, what)) for seed, what in COVER]
    for c in out:
        for a in c[1:]:
            if a is not None:
                a.setflags(write=False)
    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


def cases():
    """every directed case; read-only"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def modelled(name, mutant=None):
    """-> (ME_RESULT [n], census: the number of PUs that reached each class) of the model on the directed case `name`; computed once"""
    (_, prm, pic, ref, pus, cabac, ctb) = {c[0]: c for c in _cases()}[name]
    return M.search_pu_batch(pic, ref, pus, prm, cabac, ctb, mutant)


def killers(mutant, first_only=False):
    """the cases in which the mutant changes a result: ["name, PU k field: a != b"].  The cheap cases go first"""
    out = []
    for c in sorted(_cases(), key=lambda c: int(c[1]["algorithm"][0]) == 3 and int(c[1]["search_range"][0]) > 8):
        d = first_difference(modelled(c[0], mutant)[0], modelled(c[0])[0])
        if d:
            out.append("%s, %s" % (c[0], d))
            if first_only:
                break
    return out


def coverage(cases_):
    total = collections.Counter()
    for c in cases_:
        total += modelled(c[0])[1]
    return total


def assert_coverage(census):
    """every class of the census is reached by a PU of some case, but for the classes nothing can reach"""
    missing = [k for k in M.census_classes() if not census.get(k, 0) and k not in M.UNREACHABLE]
    assert not missing, "no case reaches: %s" % ", ".join(missing)
    assert not any(census.get(k, 0) for k in M.UNREACHABLE), "a class that cannot be reached was counted"


def first_difference(a, b):
    """-> "PU k field: a != b" for the first record in which two ME_RESULT arrays differ in one of the six fields, or None"""
    for i in range(len(a)):
        for f in FIELDS:
            if not np.array_equal(a[i][f], b[i][f]):
                return "PU %d %s: %s != %s" % (i, f, a[i][f].tolist(), b[i][f].tolist())
    return None


# ---------------------------------------------------------------- the census of the random inputs of the existing tests
def random_cases():
    """the inputs of test_gpu_parity.py::test_search_pu (all ME_CONFIGS), ::test_search_pu_mv_rdo, ::test_search_pu_flat_and_borders and
    ::test_search_pu_amp_smp_shapes, as cases (192 x 128 all)"""
    from test_gpu_parity import AMP_SMP_SHAPES, ME_CONFIGS, MV_RDO_CONFIGS
    out = []
    for cfg in range(len(ME_CONFIGS)):
        prm = me_params(**ME_CONFIGS[cfg])
        for k, motion in enumerate(((3, -2), (-7, 5), (0, 0), (14, 9))):
            pic, ref = me_frames(192, 128, 900 + k, motion)
            pus = me_pus_in_tile(me_random_pus(192, 128, 60, 177 + 10 * cfg + k, hint=(-4 * motion[0] + 2, -4 * motion[1])), prm)
            out.append(case("search_pu/%d/%d" % (cfg, k), prm, pic, ref, pus))
    for cfg in range(len(MV_RDO_CONFIGS)):
        prm = me_params(**MV_RDO_CONFIGS[cfg])
        for k, motion in enumerate(((3, -2), (-7, 5), (0, 0))):
            pic, ref = me_frames(192, 128, 900 + k, motion)
            pus = me_random_pus(192, 128, 60, 277 + 10 * cfg + k, hint=(-4 * motion[0] + 2, -4 * motion[1]),
                                sizes=((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (64, 32), (24, 32), (32, 8), (8, 4), (16, 12)))
            pus["x"], pus["y"] = np.minimum(pus["x"], 192 - pus["width"]), np.minimum(pus["y"], 128 - pus["height"])
            pus["reserved"] = np.arange(len(pus)) % 9
            out.append(case("mv_rdo/%d/%d" % (cfg, k), prm, pic, ref, pus, me_cabac_states(9, 15 + k + cfg)))
    prm = me_params(lambda_cost=3, early_termination=0)
    out.append(case("flat", prm, flat(77), flat(77), me_random_pus(192, 128, 30, 5)))
    pic, ref = me_frames(192, 128, 31, (20, -17))
    pus = me_random_pus(192, 128, 60, 6, sizes=((8, 8), (16, 16), (64, 64), (32, 32)))
    pus["x"] = np.where(np.arange(60) % 2 == 0, 0, 192 - pus["width"])
    pus["y"] = np.where(np.arange(60) % 3 == 0, 0, 128 - pus["height"])
    pus["extra_mv"] = np.array([[-130, 90], [150, -120], [4, 300]] * 20, dtype=np.int16)
    out.append(case("borders", prm, pic, ref, pus))
    for cfg in (0, 3, 4, 6, 8, 11, 14):
        prm = me_params(**ME_CONFIGS[cfg])
        for k, motion in enumerate(((3, -2), (-6, 5), (0, 0))):
            pic, ref = me_frames(192, 128, 950 + k, motion)
            pus = me_random_pus(192, 128, 64, 31 + 10 * cfg + k, hint=(-4 * motion[0] + 1, -4 * motion[1]), sizes=AMP_SMP_SHAPES)
            pus["x"] = (pus["x"] // 4) * 4 + 4 * (np.arange(len(pus)) % 2)
            pus["x"] = np.minimum(pus["x"], 192 - pus["width"])
            out.append(case("amp_smp/%d/%d" % (cfg, k), prm, pic, ref, pus))
        pic, ref = me_frames(192, 128, 33, (18, -15))
        pus = me_random_pus(192, 128, 40, 8, sizes=((4, 8), (4, 16), (12, 16), (8, 4), (16, 4), (16, 12)))
        pus["x"] = np.where(np.arange(40) % 2 == 0, 0, 192 - pus["width"])
        pus["y"] = np.where(np.arange(40) % 3 == 0, 0, 128 - pus["height"])
        pus["extra_mv"] = np.array([[-130, 90], [150, -120]] * 20, dtype=np.int16)
        out.append(case("amp_smp_borders/%d" % cfg, prm, pic, ref, pus))
    return out


def random_census(check=None):
    """-> (census of the model over random_cases(), number of PUs).  check: a library with search_pu_batch (oracle_lib, ref_lib) the model is
    compared with on the way"""
    total, n = collections.Counter(), 0
    for (name, prm, pic, ref, pus, cabac, ctb) in random_cases():
        got, census = M.search_pu_batch(pic, ref, pus, prm, cabac, ctb)
        if check is not None:
            d = first_difference(got, check.search_pu_batch(pic, ref, pus, prm, cabac=cabac, cost_to_beat=ctb))
            assert d is None, "%s: %s" % (name, d)
        total += census
        n += len(pus)
    return total, n


# ---------------------------------------------------------------- the fixture: inputs and the compiled reference's results
def build_fixture(B):
    """B: ref_lib or oracle_lib.  Integer arrays and names only; a plane many cases share is stored once"""
    planes, index = [], {}

    def plane(a):
        key = a.tobytes()
        if key not in index:
            index[key] = len(planes)
            planes.append(np.ascontiguousarray(a))
        return index[key]
    d = {"names": np.array([c[0] for c in cases()])}
    for (n, prm, pic, ref, pus, cabac, ctb) in cases():
        p = np.array(prm)
        p["cabac"], p["cost_to_beat"] = 0, 0
        d[n + "/prm"] = p.view(np.uint8)
        d[n + "/planes"] = np.array([plane(pic), plane(ref)], np.int32)
        d[n + "/pus"] = np.ascontiguousarray(pus).view(np.uint8).reshape(len(pus), 64)
        d[n + "/ctb"] = np.asarray(ctb, dtype=np.uint32)
        if cabac is not None:
            d[n + "/cabac"] = np.ascontiguousarray(cabac).view(np.uint8).reshape(len(cabac), 16)
        want = B.search_pu_batch(pic, ref, pus, prm, cabac=cabac, cost_to_beat=ctb)
        d[n + "/want"] = np.ascontiguousarray(want).view(np.uint8).reshape(len(pus), 32)
    d["planes"] = np.stack(planes)
    return d


def load_fixture(z):
    """-> [(case, want ME_RESULT [n])] as build_fixture stored them"""
    planes = z["planes"]
    out = []
    for n in z["names"]:
        n = str(n)
        k = z[n + "/planes"]
        cabac = np.ascontiguousarray(z[n + "/cabac"]).view(ME_CABAC).reshape(-1) if n + "/cabac" in z.files else None
        c = (n, np.ascontiguousarray(z[n + "/prm"]).view(ME_PARAMS), np.ascontiguousarray(planes[k[0]]), np.ascontiguousarray(planes[k[1]]),
             np.ascontiguousarray(z[n + "/pus"]).view(ME_PU).reshape(-1), cabac, np.ascontiguousarray(z[n + "/ctb"]))
        out.append((c, np.ascontiguousarray(z[n + "/want"]).view(ME_RESULT).reshape(-1)))
    return out

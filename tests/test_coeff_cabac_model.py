"""CPU: the model of the reference's CABAC coefficient pricing (tests/coeff_cabac_model.py) against the compiled reference's own counting
coder on fresh seeds (where the reference is built), against tests/golden/coeff_cabac.npz everywhere; the census and the deliberate
errors of the model; the fixture's size and that it regenerates from the cases."""
import collections
import os

import numpy as np
import pytest

import coeff_cabac_cases as K
import coeff_cabac_model as M
import ref_coeff_cost as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coeff_cabac.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def tus(f):
    for i, (off, width, type_, scan, tr_skip, set_, cfg) in enumerate(f["desc"].tolist()):
        yield i, f["coeffs"][off:off + width * width], width, type_, scan, tr_skip, set_, tuple(f["configs"][cfg].tolist())


@pytest.fixture(scope="module")
def model_run(fixture):
    """the model over the whole fixture, once: (bits, census)"""
    census = collections.Counter()
    bits = np.zeros(len(fixture["desc"]), dtype=np.uint32)
    for i, c, width, type_, scan, tr_skip, set_, (sh, ts, ll) in tus(fixture):
        bits[i] = M.count_bits(c.tolist(), width, type_, scan, tr_skip, int(fixture["ranges"][set_]), fixture["dumps"][set_].tolist(), sh, ts, ll,
                               census=census)
    return bits, census


def test_fixture_is_small_and_is_the_cases(fixture):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    coeffs, desc = K.pack(K.cases())
    ranges, dumps = K.context_sets()
    assert (fixture["coeffs"] == coeffs).all() and (fixture["desc"] == desc).all()
    assert (fixture["ranges"] == ranges).all() and (fixture["dumps"] == dumps).all() and fixture["configs"].tolist() == [list(c) for c in K.CONFIGS]
    d = fixture["desc"]
    assert (d[:, 0] % 4 == 0).all() and set(d[:, 1].tolist()) == {4, 8, 16, 32} and set(d[:, 2].tolist()) == {0, 2}
    assert {(w, s) for w, s in d[:, [1, 3]].tolist()} == {(4, 0), (4, 1), (4, 2), (8, 0), (8, 1), (8, 2), (16, 0), (32, 0)}
    assert fixture["dumps"].max() <= 125 and fixture["ranges"].min() >= 256 and fixture["ranges"].max() <= 510
    mags = np.abs(fixture["coeffs"].astype(np.int32))
    assert mags.max() == 32768 and (mags == 32767).any() and (mags == 1).any()
    assert (fixture["bits"] == 0).sum() >= 8 and fixture["bits"].max() > 20000


def test_model_gives_the_fixture_counts(fixture, model_run):
    bits, _ = model_run
    wrong = np.flatnonzero(bits != fixture["bits"])
    assert wrong.size == 0, (wrong[:8], bits[wrong[:8]], fixture["bits"][wrong[:8]])


def test_fixture_reaches_every_census_class(fixture, model_run):
    _, census = model_run
    assert set(census) <= set(M.CLASSES) and len(set(M.CLASSES)) == len(M.CLASSES)
    short = {k: census[k] for k in M.CLASSES if census[k] < 4}
    assert not short, short
    assert [census[k] for k in M.CLASSES] == fixture["census"].tolist()
    # what the census must list at the least
    for k in ("sign:hidden", "sign:not-hidden", "c1:1-to-2", "c1:2-to-3", "c1:to-0", "c1:stays-0", "greater2:coded", "greater2:not-coded",
              "group:more-than-8-non-zeros", "rice:0", "rice:1", "rice:2", "rice:3", "rice:4", "remain:prefix-le-3", "remain:escape",
              "last:x-suffix", "last:y-suffix", "last:vertical-swap", "cg:coded-1-ctx-0", "cg:coded-1-ctx-1", "cg:coded-0-ctx-0",
              "cg:coded-0-ctx-1", "cg:first-inferred", "cg:last-inferred", "pattern:0", "pattern:1", "pattern:2", "pattern:3", "sig:4x4-table",
              "sig:dc", "sig:8x8-diagonal", "sig:8x8-other-scan", "sig:larger-luma", "sig:luma-group-offset", "sig:larger-chroma", "sig:inferred",
              "ctx-set:bump", "trskip:bin-0", "trskip:absent-width", "trskip:absent-disabled", "mps:shift", "mps:no-shift", "lps:shift-1",
              "lps:shift-6", "state:saturates-at-62", "state:mps-flips-at-0"):
        assert k in M.CLASSES, k


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_deliberate_error_changes_a_stored_count(fixture, mutant):
    assert len(M.MUTANTS) >= 25
    for i, c, width, type_, scan, tr_skip, set_, (sh, ts, ll) in tus(fixture):
        got = M.count_bits(c.tolist(), width, type_, scan, tr_skip, int(fixture["ranges"][set_]), fixture["dumps"][set_].tolist(), sh, ts, ll,
                           mutant=mutant)
        if got != fixture["bits"][i]:
            return
    pytest.fail("no stored count notices %r (%s)" % (mutant, M.MUTANTS[mutant]))


def test_model_leaves_the_callers_contexts_alone(fixture):
    ctx = fixture["dumps"][7].tolist()
    before = list(ctx)
    assert M.count_bits([3, -1, 0, 2] * 4, 4, 0, 0, 0, 300, ctx) > 0 and ctx == before


@needs_ref
def test_scan_tables_are_the_references():
    for width in (4, 8, 16, 32):
        for mode in ((0, 1, 2) if width <= 8 else (0,)):
            assert R.scan_table(width, mode) == M.scan_tables(width, mode)[0], (width, mode)


@needs_ref
def test_reference_structure_is_the_documented_one():
    import ctypes
    assert ctypes.sizeof(R.CabacData) == 224 and R.CabacData.ctx.offset == 40 and R.CabacData.range.offset == 12


@needs_ref
@pytest.mark.parametrize("seed", (101, 202))
def test_model_equals_the_compiled_reference_on_fresh_seeds(seed):
    g = np.random.default_rng(seed)
    for t in range(400):
        width = int(g.choice([4, 8, 16, 32]))
        type_, scan = int(g.choice([0, 2])), int(g.integers(0, 3)) if width <= 8 else 0
        mag = int(g.choice([1, 2, 4, 20, 300, 32767]))
        c = (g.integers(-mag, mag + 1, width * width) * (g.random(width * width) < g.choice([0.02, 0.1, 0.4, 0.9]))).astype(np.int16)
        ctx, rng = g.integers(0, 126, 184).tolist(), int(g.integers(256, 511))
        sh, ts, ll, tr_skip = (int(v) for v in g.integers(0, 2, 4))
        want, after = R.coeff_cabac_cost(c, width, type_, scan, rng, ctx, sh, ts, ll, tr_skip)
        assert M.count_bits(c.tolist(), width, type_, scan, tr_skip, rng, ctx, sh, ts, ll) == want, (seed, t, width, type_, scan)
        # only the bytes a kvz_hip_coeff_ctx carries are ever touched by the reference's coder
        changed = [i for i in range(184) if after[i] != ctx[i]]
        assert all(32 <= i < 168 or i in (182, 183) for i in changed)


@needs_ref
def test_fixture_counts_are_the_compiled_references(fixture):
    step = 7                                                     # every seventh TU and all the large ones: the generator checked them all
    for i, c, width, type_, scan, tr_skip, set_, (sh, ts, ll) in tus(fixture):
        if i % step and width < 16:
            continue
        want, _ = R.coeff_cabac_cost(c, width, type_, scan, int(fixture["ranges"][set_]), fixture["dumps"][set_], sh, ts, ll, tr_skip)
        assert want == fixture["bits"][i], i

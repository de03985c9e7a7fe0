"""CPU: the plain model of the deblocking filter (tests/deblock_model.py) and the directed pictures (tests/deblock_directed_cases.py).
The model equals the oracle -- and the compiled reference where it was built -- on every directed picture and on the random pictures of
both deblocking tests; the directed pictures reach every class of the model's census on at least 8 segments in each direction; every
mutant of the model changes the result on one of them, in each direction; and the committed fixture
tests/golden/deblock_directed.npz, which the GPU test compares with, is what the model and the oracle give."""
import os

import numpy as np
import pytest

import deblock_directed_cases as DC
import deblock_model as M
import oracle_lib as O
import ref_lib as R
import tile_chain_cases as TC
from test_gpu_parity import DEBLOCK_CONFIGS as GPU_CONFIGS
from test_oracle_vs_ref import DEBLOCK_CONFIGS as REF_CONFIGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deblock_directed.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")
NAMES = [c["name"] for c in DC.cases()]
CASES = {c["name"]: c for c in DC.cases()}


def same(got, want, what):
    for k in range(3):
        assert (got[k] is None) == (want[k] is None), what
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s, plane %d" % (what, k))


def test_the_two_profiles_of_the_empty_classes():
    """the strong filter clips p0 at +2 tc, and the weak filter would make q0 256"""
    md = M._Model(np.zeros((8, 8), np.uint8), None, None, np.zeros((2, 2), DC.CU_INFO), DC.deblock_params(chroma=0), None, None, None)
    b = [[105, 105, 105, 100, 102, 102, 102, 102] for _ in range(4)]
    assert md.luma_segment(b, 50, 1) == {"strong:clip+"} and b[0] == [105, 104, 103, 102, 102, 102, 102, 102]
    b = [[247, 250, 250, 255, 255, 255, 255, 255] for _ in range(4)]
    assert "weak:p0q0-clamp255" in md.luma_segment(b, 64, 4) and b[0][3:5] == [254, 255]


def test_directed_pictures_are_small_and_of_every_kind():
    cases = DC.cases()
    assert len(cases) == 24 and len(set(NAMES)) == 24
    for c in cases:
        h, w = c["y"].shape
        assert max(w, h) <= 192 and min(w, h) <= 128 and w % 8 == 0 and h % 8 == 0
        assert c["cus"].shape == (h // 4, w // 4) and (c["u"] is None) == (not c["prm"]["chroma"][0])
    assert CASES["strong"]["u"] is None and CASES["tiles"]["col_bd"] == [0, 1, 2] and CASES["tiles"]["row_bd"] == [0, 1, 2]
    assert CASES["bs-b"]["prm"]["slice_is_b"][0] == 1 and CASES["qp"]["prm"]["per_cu_qp"][0] == 1
    q = CASES["qp"]["cus"]["qp"].astype(int)
    assert (np.abs(np.diff(q, axis=1)) % 2 == 1).any()
    assert (CASES["amp^T"]["cus"]["part_size"][0, :8] == 4).all() and (CASES["amp"]["cus"]["part_size"][0, :8] == 6).all()


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_on_a_directed_picture(name):
    c = CASES[name]
    got, census = DC.modelled(name)
    same(got, DC.expected(c, O), name + ": model against the oracle")
    if c["col_bd"] is None:
        same(got, O.deblock_frame(c["y"], c["u"], c["v"], c["cus"], c["prm"]), name)
    else:
        same(got, TC.deblock((c["y"], c["u"], c["v"]), c["cus"], c["prm"], c["col_bd"], c["row_bd"]), name + ": tile_chain_cases.deblock")
        whole = M.deblock(c["y"], c["u"], c["v"], c["cus"], c["prm"])[0]
        assert DC.first_difference(got, whole) is not None, "the tile boundaries carry nothing that the untiled filter would change"
        assert census["v:tile:skipped"] >= DC.COVERAGE_MIN or census["h:tile:skipped"] >= DC.COVERAGE_MIN


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_compiled_reference_on_a_directed_picture(name):
    same(DC.modelled(name)[0], DC.expected(CASES[name], R), name + ": model against the compiled reference")


@pytest.mark.parametrize("which", ["gpu test", "oracle test"])
def test_model_equals_the_oracle_on_the_random_pictures(which):
    configs, first_seed = (GPU_CONFIGS, 300) if which == "gpu test" else (REF_CONFIGS, 100)
    assert tuple(GPU_CONFIGS) == DC.RANDOM_CONFIGS
    total = M.collections.Counter()
    for c in DC.random_cases(tuple(configs), first_seed):
        got, census = M.deblock(c["y"], c["u"], c["v"], c["cus"], c["prm"])
        total += census
        same(got, O.deblock_frame(c["y"], c["u"], c["v"], c["cus"], c["prm"]), c["name"])
        if R.available():
            same(got, R.deblock_frame(c["y"], c["u"], c["v"], c["cus"], c["prm"]), c["name"] + ": compiled reference")
    # what these pictures leave to the directed ones (a figure, not a requirement: the random pictures are what they are)
    print("classes on fewer than %d segments: %s" % (DC.COVERAGE_MIN, ", ".join("%s %d" % (k, total.get(k, 0)) for k in M.census_classes()
                                                                                 if total.get(k, 0) < DC.COVERAGE_MIN)))


def test_directed_pictures_reach_every_class_in_each_direction():
    census = DC.coverage(DC.cases())
    DC.assert_coverage(census)
    assert len(M.census_classes()) == 2 * len(M.LUMA_CLASSES) + len(M.H_ONLY_CLASSES) + 4 * len(M.CHROMA_CLASSES)
    # the threshold is a threshold: a census without one class, or with 7 segments of it, is refused
    for k in ("v:strong:clip+", "h:u:chroma:clamp255"):
        short = M.collections.Counter(census)
        short[k] = DC.COVERAGE_MIN - 1
        with pytest.raises(AssertionError, match=k):
            DC.assert_coverage(short)


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_mutant_changes_a_directed_picture_in_each_direction(mutant):
    for direction, suffix in (("vertical", ""), ("horizontal", "^T")):
        killed = []
        for name in NAMES:
            if name.endswith("^T") == bool(suffix):
                d = DC.first_difference(DC.modelled(name, mutant)[0], DC.modelled(name)[0])
                if d:
                    killed.append("%s, %s" % (name, d))
        assert killed, "%s (%s) changes no picture of the %s set" % (mutant, M.MUTANTS[mutant], direction)
        print("%s, %s set: %s" % (mutant, direction, killed[0]))


def test_fixture_is_what_the_model_and_the_oracle_give():
    assert os.path.getsize(GOLDEN) < 400 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "uiU" for k in z.files)
    fresh = DC.build_fixture(O)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)
    loaded = DC.load_fixture(z)
    assert [c["name"] for c, _ in loaded] == NAMES
    for c, want in loaded:
        same(DC.modelled(c["name"])[0], want, c["name"] + ": model against the fixture")
        same(M.deblock(c["y"], c["u"], c["v"], c["cus"], c["prm"], c["col_bd"], c["row_bd"])[0], want, c["name"] + ": the loaded inputs")


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    z = np.load(GOLDEN, allow_pickle=False)
    fresh = DC.build_fixture(R)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)

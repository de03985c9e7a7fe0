"""CPU: the plain model of the merge / AMVP candidate derivation (tests/inter_cand_model.py) and the directed CU maps
(tests/inter_cand_directed_cases.py).  The model equals the oracle -- and the compiled reference where it was built -- on every directed
case, on the random cases of both existing candidate tests, on the recorded encoder states and on the reference's known answers; the
directed cases reach every class of the model's census on at least 4 PUs; every mutant of the model changes the result of one of them;
and the committed fixture tests/golden/inter_cand_directed.npz, which the GPU test compares with, is what the model and the oracle give."""
import collections
import os

import numpy as np
import pytest

import inter_cand_directed_cases as DC
import inter_cand_model as M
import oracle_lib as O
import ref_lib as R
from patterns import (CU_INFO, INTER_CAND_CONFIGS, ME_PU, MV_CAND_KAT_A0, MV_CAND_KAT_B0, MV_CAND_KAT_SPATIAL, inter_params,
                      recorded_cand_fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_cand_directed.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")
NAMES = [c[0] for c in DC.cases()]
CASES = {c[0]: c for c in DC.cases()}


def same(got, want, what):
    d = DC.first_difference(got[:2], want)
    assert d is None, "%s: %s" % (what, d)
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(np.asarray(got[1]).view(np.uint8), np.asarray(want[1]).view(np.uint8), err_msg=what)


def test_directed_cases_are_small_and_of_every_kind():
    cases = DC.cases()
    assert 20 <= len(cases) <= 30
    prm = {n: c[1][0] for n, c in CASES.items()}
    for (name, p, cus, col, ref_cus, pus) in cases:
        assert int(p["pic_width"][0]) <= 192 and int(p["pic_height"][0]) <= 136 and len(pus) <= 256, name
        assert cus.shape[1] == p["cus_stride"][0] > (int(p["pic_width"][0]) + 63) // 64 * 16, name
        assert col.shape[1] == p["col_stride"][0] > (int(p["in_width"][0]) + 63) // 64 * 16, name
        for m in (cus, col, ref_cus):                        # record 0 is not set and carries a wild vector
            assert m is None or (m[0, 0]["type"] == 0 and abs(int(m[0, 0]["mv"][0, 0])) >= 9000), name
        x, y = pus["x"] - p["tile_x"][0], pus["y"] - p["tile_y"][0]
        assert (x >= 0).all() and (y >= 0).all() and (x + pus["width"] <= p["pic_width"][0]).all() and (y + pus["height"] <= p["pic_height"][0]).all()
        assert len(pus) < 8 or (np.diff(pus["y"].astype(int) * 1000 + pus["x"]) < 0).any(), name + ": the PUs are not in raster order"
    assert sum(len(c[5]) % 64 != 0 for c in cases) >= 2
    assert any(c[1]["pic_width"][0] == 192 and c[1]["pic_height"][0] == 136 for c in cases)
    assert (prm["p-tile-64-0"]["tile_x"], prm["p-tile-64-0"]["tile_y"], prm["p-tile-64-0"]["slice_is_b"]) == (64, 0, 0)
    assert (prm["b-tile-64-64"]["tile_x"], prm["b-tile-64-64"]["tile_y"], prm["b-tile-64-64"]["slice_is_b"]) == (64, 64, 1)
    assert prm["p-one-ref"]["num_refs"] == 1 and prm["p-three-refs"]["num_refs"] == 3 and prm["p-no-tmvp"]["tmvp_enable"] == 0 and prm["p-poc-1"]["poc"] == 1
    assert (CASES["p-col-intra"][3]["type"][:18, :32] != 2).all()
    assert CASES["p-no-ref-cus"][4] is None and CASES["b-no-ref-cus"][4] is None
    # every partition mode: the shapes of its PUs, and both barred neighbours
    shapes = {(int(w), int(h)) for c in cases for w, h in zip(c[5]["width"], c[5]["height"])}
    for n in (16, 32):
        assert {(n, n), (n, n // 2), (n // 2, n), (n, n // 4), (n, 3 * n // 4), (n // 4, n), (3 * n // 4, n)} <= shapes
    assert {(8, 8), (8, 4), (4, 8)} <= shapes
    assert {int(v) for c in cases for v in c[5]["pad"]} == {0, 1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_on_a_directed_case(name):
    same(DC.modelled(name), O.inter_candidates(*CASES[name][1:]), name + ": model against the oracle")


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_compiled_reference_on_a_directed_case(name):
    same(DC.modelled(name), R.inter_candidates(*CASES[name][1:]), name + ": model against the compiled reference")


@pytest.mark.parametrize("which", ["gpu test", "oracle test"])
def test_model_equals_the_oracle_on_the_random_cases(which):
    cases = DC.random_cases(which)
    assert {c[0].split("/")[0] for c in cases} == {c[0] for c in INTER_CAND_CONFIGS}
    total, results = collections.Counter(), {}
    for c in cases:
        got = M.derive(*c[1:])
        total += got[2]
        results[c[0]] = got[:2]
        same(got, O.inter_candidates(*c[1:]), c[0])
        if R.available():
            same(got, R.inter_candidates(*c[1:]), c[0] + ": compiled reference")
    # what these cases leave to the directed ones (figures, not requirements: the random cases are what they are)
    print("%s, %d PUs: classes on fewer than %d PUs: %s" % (which, sum(len(c[5]) for c in cases), DC.COVERAGE_MIN, ", ".join(
        "%s %d" % (k, total.get(k, 0)) for k in M.census_classes() if total.get(k, 0) < DC.COVERAGE_MIN)))
    by_seed = sorted(cases, key=lambda c: int(c[0].split("/")[1]))         # one case of every configuration first: most mutants end there
    alive = [m for m in sorted(M.MUTANTS) if not any(DC.first_difference(M.derive(*c[1:], mutant=m)[:2], results[c[0]]) for c in by_seed)]
    print("%s: mutants that change none of these cases: %s" % (which, ", ".join(alive)))


def test_model_gives_the_recorded_candidates():
    """candidates the reference encoder derived during a real encode (tests/golden/recorded_cand.npz)"""
    z = np.load(os.path.join(os.path.dirname(GOLDEN), "recorded_cand.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}                           # read once: the fixture function asks for its arrays at every record
    got, want = recorded_cand_fixture(d, lambda *a: M.derive(*a)[0])
    for fld in ("num_merge_cand", "merge", "mv_cand", "extra_mv"):
        np.testing.assert_array_equal(got[fld], want[fld], err_msg=fld)


def test_model_gives_the_known_answers_of_the_reference():
    """tests/mv_cand_tests.c: the truth tables of the two coding-order tests, and the places of the five neighbours in lcu_t.cu"""
    md = M._Model(inter_params(64, 64), None, None, None, None)
    assert [md.a0_coded(*g) for g, _ in MV_CAND_KAT_A0] == [e for _, e in MV_CAND_KAT_A0]
    assert [md.b0_coded(*g) for g, _ in MV_CAND_KAT_B0] == [e for _, e in MV_CAND_KAT_B0]
    (x, y, w, h, pic_w, pic_h), want = MV_CAND_KAT_SPATIAL
    p = inter_params(pic_w, pic_h, tmvp=0)
    cus = np.zeros(((pic_h + 63) // 64 * 16, int(p["cus_stride"][0])), CU_INFO)
    cus["type"], cus["mv_dir"] = 2, 1
    rows, cols = np.mgrid[0:cus.shape[0], 0:cus.shape[1]]
    cus["mv"][..., 0, 0], cus["mv"][..., 0, 1] = cols, rows              # every record names its place
    md = M._Model(p, cus, None, None, None)
    md.hits = set()
    c = md.spatial(x, y, w, h)

    def lcu_index(cand):
        """the record's index in lcu_t.cu (cu.h:324-344): 17 x 17 records from the corner above and left of the LCU, then the top-right one"""
        sx, sy = cand[1][0][0] - (x // 64) * 16, cand[1][0][1] - (y // 64) * 16
        return 289 if sx == 16 else 18 + sx + 17 * sy
    assert tuple(lcu_index(c[k]) for k in ("b0", "b1", "b2", "a0", "a1")) == want


def test_directed_cases_reach_every_class():
    census = DC.coverage(DC.cases())
    DC.assert_coverage(census)
    assert len(M.census_classes()) == len(set(M.census_classes())) >= 130
    # the threshold is a threshold: a census without one class, or with 3 PUs of it, is refused
    for k, n in (("merge:pair-11:taken", 0), ("scale:scale-min", DC.COVERAGE_MIN - 1)):
        short = collections.Counter(census)
        short[k] = n
        with pytest.raises(AssertionError, match=k):
            DC.assert_coverage(short)
    # the two classes the reference's code cannot reach are reached by nothing
    assert not any(census.get(k, 0) for k in M.UNREACHABLE)


def test_mutants_are_enough_and_of_every_group():
    assert len(M.MUTANTS) >= 30
    groups = collections.Counter(M.MUTANT_GROUP.values())
    assert set(groups) == set(M.GROUPS) and min(groups.values()) >= 3, groups


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_mutant_changes_a_directed_case(mutant):
    killed = []
    for name in NAMES:
        d = DC.first_difference(DC.modelled(name, mutant)[:2], DC.modelled(name)[:2])
        if d:
            killed.append("%s, %s" % (name, d))
    assert killed, "%s (%s) changes no directed case" % (mutant, M.MUTANTS[mutant])
    print("%s: %d cases, first %s" % (mutant, len(killed), killed[0]))


def test_fixture_is_what_the_model_and_the_oracle_give():
    assert os.path.getsize(GOLDEN) < 400 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "uiU" for k in z.files)
    fresh = DC.build_fixture(O)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)
    loaded = DC.load_fixture(z)
    assert [c[0] for c, _, _ in loaded] == NAMES
    for c, want_pus, want_merge in loaded:
        assert want_pus.dtype == ME_PU and want_merge.shape == (len(c[5]), 5)
        same(DC.modelled(c[0]), (want_pus, want_merge), c[0] + ": model against the fixture")
        same(M.derive(*c[1:]), (want_pus, want_merge), c[0] + ": the loaded inputs")


@needs_ref
def test_fixture_regenerates_from_the_compiled_reference():
    z = np.load(GOLDEN, allow_pickle=False)
    fresh = DC.build_fixture(R)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)

"""CPU: the plain model of the motion search (tests/me_search_model.py) and the directed cases (tests/me_search_directed_cases.py).  On the
committed fixture tests/golden/me_search_directed.npz, which the GPU test compares with: the model gives what it holds, the oracle gives what
it holds, the compiled reference -- where it was built -- still gives what it holds; the cases reach every class of the model's census;
every mutant of the model changes the result of one of them."""
import collections
import functools
import os

import numpy as np
import pytest

import me_search_directed_cases as DC
import me_search_model as M
import oracle_lib as O
import ref_lib as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_search_directed.npz")
needs_ref = pytest.mark.skipif(not R.available(), reason="compiled reference not built")
NAMES = [c[0] for c in DC.cases()]


@functools.lru_cache(maxsize=None)
def fixture():
    return tuple(DC.load_fixture(np.load(GOLDEN, allow_pickle=False)))


def same(got, want, what):
    d = DC.first_difference(got, want)
    assert d is None, "%s: %s" % (what, d)


def test_fixture_holds_the_directed_cases_and_data_only():
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "uiU" for k in z.files)
    assert [c[0] for c, _ in fixture()] == NAMES
    for (c, want), mine in zip(fixture(), DC.cases()):
        assert c[2].shape == c[3].shape == (DC.H, DC.W) == (128, 192), c[0]
        for a, b in zip(c[1:], mine[1:]):
            assert (a is None) == (b is None), c[0]
            if a is not None and a.dtype.names and "cabac" in a.dtype.names:         # the parameters travel without their two addresses
                b = np.array(b)
                b["cabac"], b["cost_to_beat"] = 0, 0
            assert a is None or a.tobytes() == b.tobytes(), c[0]
        assert len(want) == len(c[4]) <= 12
    total = sum(len(c[4]) for c, _ in fixture())
    assert 200 <= total <= 600, total
    big = [c[0] for c, _ in fixture() if c[1]["algorithm"][0] == 3 and c[1]["search_range"][0] == 64]
    assert big == ["full-lds-64-r64"] and len(fixture()[NAMES.index(big[0])][0][4]) == 1


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_fixture(name):
    c, want = fixture()[NAMES.index(name)]
    same(DC.modelled(name)[0], want, name + ": model on the module's case")
    same(M.search_pu_batch(c[2], c[3], c[4], c[1], c[5], c[6])[0], want, name + ": model on the loaded inputs")


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_fixture(name):
    c, want = fixture()[NAMES.index(name)]
    same(O.search_pu_batch(c[2], c[3], c[4], c[1], cabac=c[5], cost_to_beat=c[6]), want, name + ": oracle")


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_compiled_reference_equals_the_fixture(name):
    c, want = fixture()[NAMES.index(name)]
    same(R.search_pu_batch(c[2], c[3], c[4], c[1], cabac=c[5], cost_to_beat=c[6]), want, name + ": compiled reference")


def test_directed_cases_reach_every_class():
    census = DC.coverage(DC.cases())
    DC.assert_coverage(census)
    classes = M.census_classes()
    assert len(classes) == len(set(classes)) >= 300
    # a census without one class is refused
    for k in ("tie:hex3:first-wins", "cost:golomb:fallback-y"):
        short = collections.Counter(census)
        short[k] = 0
        with pytest.raises(AssertionError, match=k.replace("^", ".")):
            DC.assert_coverage(short)
    # the classes nothing can reach are few, argued, and reached by nothing
    assert len(M.UNREACHABLE) <= 4 and set(M.UNREACHABLE) <= set(classes) and all(len(v) > 40 for v in M.UNREACHABLE.values())
    assert not any(census.get(k, 0) for k in M.UNREACHABLE)
    # the exhaustive-search windows around the LDS bound of each size class, from frac_geom, not by trial
    assert (M.win_bytes(16), M.win_bytes(32), M.win_bytes(64)) == (4192, 12128, 40288)
    assert M.window_fits(64, 64, 64) and not M.window_fits(32, 32, 64) and not M.window_fits(16, 16, 32) and M.window_fits(8, 8, 8)


def test_random_cases_of_the_existing_tests_leave_classes_out():
    """a sample of what the docstring of the cases module counts over all of them: one picture pair of every configuration of
    test_search_pu; the model equals the oracle there too"""
    total = collections.Counter()
    for c in [c for c in DC.random_cases() if c[0].startswith("search_pu/") and c[0].endswith("/0")][::3]:
        got, census = M.search_pu_batch(c[2], c[3], c[4][:20], c[1], c[5], c[6][:20])
        same(got, O.search_pu_batch(c[2], c[3], c[4][:20], c[1], cabac=c[5], cost_to_beat=c[6][:20]), c[0])
        total += census
    for k in ("cost:golomb:fallback-x", "cost:merge:wrapped-equal-outside-int16", "et:l2:equal-threshold", "cost:lambda:2^20", "hex:steps:zero"):
        assert not total.get(k), k


def test_mutants_are_enough_and_of_every_group():
    assert len(M.MUTANTS) >= 40
    groups = collections.Counter(M.MUTANT_GROUP.values())
    assert set(groups) == set(M.GROUPS) and min(groups.values()) >= 2, groups
    for must in ("last-wins", "le-incumbent", "wpp-floor-division", "merge-no-range-check", "golomb-fast-past-2^16", "hex-wrap1", "hex-wrap8",
                 "tz-rounds-2", "tz-second-run-from-start", "full-jump-plus-one", "full-unusable-window-counted", "gate-le", "c3-with-c4-margins"):
        assert must in M.MUTANTS


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_mutant_changes_a_directed_case(mutant):
    killed = DC.killers(mutant, first_only=True)
    assert killed, "%s (%s) changes no directed case" % (mutant, M.MUTANTS[mutant])
    print("%s: %s" % (mutant, killed[0]))


def test_fixture_is_what_the_oracle_gives():
    z = np.load(GOLDEN, allow_pickle=False)
    fresh = DC.build_fixture(O)
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        np.testing.assert_array_equal(z[k], fresh[k], err_msg=k)

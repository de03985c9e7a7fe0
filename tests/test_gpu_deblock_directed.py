"""GPU: the three entries of deblock_pass_kernel -- kvz_hip_deblock_frame, kvz_hip_deblock_frame_tiles and kvz_hip_deblock_frames -- on
the directed pictures of tests/golden/deblock_directed.npz (tests/deblock_directed_cases.py): pictures that reach every decision of the
filter in each direction, with what the compiled reference makes of them.  On the CPU the plain model, the oracle and the reference
agree on that fixture (test_deblock_model.py), so a difference here is the kernel's.  Every plane lies inside a poisoned buffer whose
stride exceeds the width (patterns.plane_layout A and B in turn); every comparison is exact, and the poison must still be there."""
import faulthandler
import functools
import os
import sys

import numpy as np
import pytest

import deblock_directed_cases as DC
from patterns import embed_plane, plane_layout

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deblock_directed.npz")
TEST_LIMIT_S = 60                                                     # every test takes a second or two
FAULTS = []


@pytest.fixture(autouse=True)
def limits():
    assert not FAULTS, "an earlier test met a device error (%s): nothing more is started" % FAULTS[0]
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True, file=sys.__stderr__)   # the real stderr under every capture mode
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


def guarded(what, call):
    try:
        return call()
    except Exception:
        FAULTS.append(what)
        raise


@functools.lru_cache(maxsize=None)
def fixture():
    """[(case, expected planes)], loaded once and never changed"""
    return tuple(DC.load_fixture(np.load(GOLDEN, allow_pickle=False)))


NAMES = [c["name"] for c in DC.cases()]


def embedded(case, k):
    """the planes of picture k inside poisoned buffers: Y on the layout's first stride, U and V on its second one for their width"""
    layout = "AB"[k & 1]
    h, w = case["y"].shape
    sy, left, top = plane_layout(layout, w, 0)
    sc, _, _ = plane_layout(layout, w // 2, 1)
    assert sy > w and sc > w // 2 and sy % 4 == 0 and sc % 4 == 0
    return [embed_plane(p, s, left, top, 7000 + 10 * k + i, span=sy) if p is not None else None
            for i, (p, s) in enumerate(((case["y"], sy), (case["u"], sc), (case["v"], sc)))]


def views(api, emb):
    return [api.PlaneView(e.buf, e.width, e.height, e.left, e.top) if e is not None else None for e in emb]


def grid_of(api, case, one_tile=False):
    h, w = case["y"].shape
    if one_tile or case["col_bd"] is None:
        return api.tile_grid(w, h, [0, (w + 63) // 64], [0, (h + 63) // 64])
    return api.tile_grid(w, h, case["col_bd"], case["row_bd"])


def assert_result(emb, got, want, what):
    changed = False
    for k, e in enumerate(emb):
        if e is None:
            assert got[k] is None and want[k] is None, what
            continue
        np.testing.assert_array_equal(e.crop(got[k]), want[k], err_msg="%s, plane %d" % (what, k))
        assert e.poison_intact(got[k]), "%s: bytes around plane %d were written" % (what, k)
        changed = changed or bool((want[k] != e.crop()).any())
    return changed


def test_fixture_holds_the_directed_pictures():
    assert [c["name"] for c, _ in fixture()] == NAMES and len(NAMES) == 24
    kinds = {(c["col_bd"] is not None, c["u"] is None) for c, _ in fixture()}
    assert kinds == {(False, False), (False, True), (True, False)}
    # all but the pictures whose whole point is a filter that stays off are changed by the filter
    unchanged = [c["name"] for c, want in fixture() if all(want[k] is None or (want[k] == c["yuv"[k]]).all() for k in range(3))]
    assert unchanged == ["low", "floor", "low^T", "floor^T"]


@pytest.mark.parametrize("k", range(24), ids=NAMES)
def test_deblock_frame(api, k):
    case, want = fixture()[k]
    emb = embedded(case, k)
    if case["col_bd"] is None:
        got = guarded("deblock_frame", lambda: api.deblock_frame(*views(api, emb), case["cus"], case["prm"]))
        assert_result(emb, got, want, case["name"] + ": deblock_frame")
    else:
        # without its grid the tiled picture is another picture: the untiled entry filters the tile boundaries
        got = guarded("deblock_frame", lambda: api.deblock_frame(*views(api, emb), case["cus"], case["prm"]))
        assert any((e.crop(got[i]) != want[i]).any() for i, e in enumerate(emb))
        twin = {c["name"]: w_ for c, w_ in fixture()}[case["name"].replace("tiles", "untiled")]
        assert_result(emb, got, twin, case["name"] + ": deblock_frame equals the untiled twin")


@pytest.mark.parametrize("k", range(24), ids=NAMES)
def test_deblock_frame_tiles_with_one_tile(api, k):
    case, want = fixture()[k]
    if case["col_bd"] is not None:
        want = {c["name"]: w_ for c, w_ in fixture()}[case["name"].replace("tiles", "untiled")]
    emb = embedded(case, k + 1)
    got = guarded("deblock_frame_tiles", lambda: api.deblock_frame(*views(api, emb), case["cus"], case["prm"], tiles=grid_of(api, case, one_tile=True)))
    assert_result(emb, got, want, case["name"] + ": deblock_frame_tiles, one tile")


@pytest.mark.parametrize("name", ["tiles", "tiles^T"])
def test_deblock_frame_tiles_with_the_grid(api, name):
    k = NAMES.index(name)
    case, want = fixture()[k]
    assert case["col_bd"] == [0, 1, 2] and case["row_bd"] == [0, 1, 2]
    emb = embedded(case, k)
    got = guarded("deblock_frame_tiles", lambda: api.deblock_frame(*views(api, emb), case["cus"], case["prm"], tiles=grid_of(api, case)))
    assert assert_result(emb, got, want, name + ": deblock_frame_tiles, 2 x 2 tiles")


@pytest.mark.parametrize("first", [0, 8])
def test_deblock_frames_sixteen_pictures_a_call(api, first):
    """sixteen records a call, each with its own parameters: tiled beside untiled, 4:0:0 beside 4:2:0, 64 to 128 lines beside each other"""
    picked = fixture()[first:first + 16]
    assert len(picked) == 16 and any(c["col_bd"] is not None for c, _ in picked) and any(c["u"] is None for c, _ in picked)
    assert len({c["prm"].tobytes() for c, _ in picked}) >= 8
    embs = [embedded(c, first + i + 2) for i, (c, _) in enumerate(picked)]
    pictures = []
    for (c, _), emb in zip(picked, embs):
        y, u, v = views(api, emb)
        pictures.append(dict(y=y, u=u, v=v, cus=c["cus"], prm=c["prm"], tiles=grid_of(api, c) if c["col_bd"] is not None else None))
    got = guarded("deblock_frames", lambda: api.deblock_frames(pictures))
    assert len(got) == 16
    for (c, want), emb, g in zip(picked, embs, got):
        assert_result(emb, g, want, c["name"] + ": deblock_frames")

"""GPU: the motion search on the directed cases of tests/golden/me_search_directed.npz (tests/me_search_directed_cases.py): cases that reach
every decision of search_pu_core and its cost model, with what the compiled reference makes of them.  On the CPU the plain model, the oracle
and the reference agree on that fixture (test_me_search_model.py), so a difference here is the kernel's.  Every case goes through every
route: kvz_hip_search_pu_batch (search_pu_rdo_kernel for the --mv-rdo cases), the same with an availability rule that refuses nothing (the
CONSTR build), kvz_hip_search_pu_multi_batch with the plane pairs of several cases in a call, a size-class hint, and the search service
(launches and resident workers, full_qsad at both values).  All six result fields are compared; `results` holds a poison byte before
every call.  The tests read the fixture only."""
import faulthandler
import functools
import os
import sys

import numpy as np
import pytest

from patterns import ME_CABAC, ME_PARAMS, ME_PU, ME_REQUEST, ME_RESULT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_search_directed.npz")
TEST_LIMIT_S = 60                                                     # every test takes a second or two
POISON = 0xA5
MAX_INT = 2147483647
FIELDS = ("mv", "cost", "bitcost", "merged", "merge_idx", "mv_cand")
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
    """[(case, expected ME_RESULT)] as (name, params, picture, reference, PUs, snapshots or None, costs to beat); loaded once, read-only"""
    z = np.load(GOLDEN, allow_pickle=False)
    planes = z["planes"]
    out = []
    for n in z["names"]:
        n = str(n)
        k = z[n + "/planes"]
        cabac = np.ascontiguousarray(z[n + "/cabac"]).view(ME_CABAC).reshape(-1) if n + "/cabac" in z.files else None
        c = (n, np.ascontiguousarray(z[n + "/prm"]).view(ME_PARAMS), np.ascontiguousarray(planes[k[0]]), np.ascontiguousarray(planes[k[1]]),
             np.ascontiguousarray(z[n + "/pus"]).view(ME_PU).reshape(-1), cabac, np.ascontiguousarray(z[n + "/ctb"]))
        want = np.ascontiguousarray(z[n + "/want"]).view(ME_RESULT).reshape(-1)
        for a in c[1:] + (want,):
            if a is not None:
                a.setflags(write=False)
        out.append((c, want))
    return tuple(out)


def _names():
    return [str(n) for n in np.load(GOLDEN, allow_pickle=False)["names"]]


NAMES = _names()


def same(got, want, what):
    got = np.ascontiguousarray(got).view(ME_RESULT).reshape(-1)
    assert len(got) == len(want), what
    for i in range(len(want)):
        for f in FIELDS:
            assert np.array_equal(got[i][f], want[i][f]), "%s: PU %d %s: %s != %s (expected %s)" % (what, i, f, got[i][f].tolist(), want[i][f].tolist(),
                                                                                                      want[i].tolist())


def launch(api, prm, pics, refs, pus, cabac, ctb, multi=False):
    """kvz_hip_search_pu_batch, or kvz_hip_search_pu_multi_batch over the plane pairs, into a poisoned result buffer -> ME_RESULT [count]"""
    from kvazaar_amd import _lib
    L = _lib.init()
    D = api.DeviceBuffer
    prm = np.array(prm)
    keep = [D.from_numpy(np.ascontiguousarray(ctb, dtype=np.uint32))]
    prm["cost_to_beat"] = keep[0].ptr
    if cabac is not None:
        keep.append(D.from_numpy(np.ascontiguousarray(cabac).view(np.uint8)))
        prm["cabac"], prm["n_cabac"] = keep[-1].ptr, len(cabac)
    d_pics, d_refs = [D.from_numpy(p) for p in pics], [D.from_numpy(r) for r in refs]
    d_pus = D.from_numpy(np.ascontiguousarray(pus).view(np.uint8))
    out = D.from_numpy(np.full(32 * len(pus), POISON, np.uint8))
    h, w = pics[0].shape
    if multi:
        tp, tr = D.from_numpy(np.array([b.ptr for b in d_pics], np.uint64)), D.from_numpy(np.array([b.ptr for b in d_refs], np.uint64))
        api.check(L.kvz_hip_search_pu_multi_batch(tp.ptr, w, w, h, tr.ptr, w, w, h, len(pics), d_pus.ptr, len(pus), prm.ctypes.data, out.ptr, None),
                  "search_pu multi batch")
    else:
        api.check(L.kvz_hip_search_pu_batch(d_pics[0].ptr, w, w, h, d_refs[0].ptr, w, w, h, d_pus.ptr, len(pus), prm.ctypes.data, out.ptr, None),
                  "search_pu batch")
    return out.to_numpy(np.uint8, (len(pus), 32)).view(ME_RESULT).reshape(-1)


def classes_of(pus):
    w, h = pus["width"], pus["height"]
    cls = np.where((w > 32) | (h > 32), 4, np.where((w > 16) | (h > 16), 2, 1))
    return int(np.bitwise_or.reduce(cls))


def test_fixture_is_complete():
    fx = fixture()
    assert len(fx) == len(NAMES) >= 80 and 200 <= sum(len(c[4]) for c, _ in fx) <= 600
    assert all(c[2].shape == (128, 192) and c[3].shape == (128, 192) for c, _ in fx)
    assert {int(c[1]["algorithm"][0]) for c, _ in fx} == {0, 1, 2, 3} and sum(int(c[1]["mv_rdo"][0]) for c, _ in fx) >= 6
    assert {classes_of(c[4][i:i + 1]) for c, _ in fx for i in range(len(c[4]))} == {1, 2, 4}


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_search_pu_batch(api, k):
    """kvz_hip_search_pu_batch; for a --mv-rdo case that is search_pu_rdo_kernel"""
    (name, prm, pic, ref, pus, cabac, ctb), want = fixture()[k]
    same(guarded("search_pu_batch", lambda: launch(api, prm, [pic], [ref], pus, cabac, ctb)), want, name)


# the cases without a rule of their own (the RDO kernel always carries the rule)
FREE = [k for k, (c, _) in enumerate(fixture()) if not (c[1]["wpp_owf"][0] or c[1]["mv_constraint"][0] or c[1]["mv_rdo"][0])]


@pytest.mark.parametrize("k", FREE, ids=[NAMES[k] for k in FREE])
def test_search_pu_batch_with_a_rule_that_refuses_nothing(api, k):
    """a case without a constraint, run with wpp_owf = 1 and bounds no vector reaches: the CONSTR build, the same results"""
    (name, prm, pic, ref, pus, cabac, ctb), want = fixture()[k]
    assert len(FREE) >= 40
    p = np.array(prm)
    p["wpp_owf"], p["ref_delay_px"], p["max_ref_lcu_down"], p["max_ref_lcu_right"] = 1, 0, 1000, 1000
    assert p["tile_x"][0] % 64 == 0 and p["tile_y"][0] % 64 == 0
    same(guarded("search_pu_batch, inactive rule", lambda: launch(api, p, [pic], [ref], pus, cabac, ctb)), want, name + ": inactive rule")


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_search_pu_batch_with_the_size_class_hint(api, k):
    """size_classes names exactly the classes of the case's PUs"""
    (name, prm, pic, ref, pus, cabac, ctb), want = fixture()[k]
    p = np.array(prm)
    p["size_classes"] = classes_of(pus)
    same(guarded("search_pu_batch, size classes", lambda: launch(api, p, [pic], [ref], pus, cabac, ctb)), want, name + ": size_classes %d" % p["size_classes"][0])


def multi_groups():
    """the cases without --mv-rdo (the entry refuses it), grouped by their parameters: a call per group"""
    groups = {}
    for k, (c, _) in enumerate(fixture()):
        if not c[1]["mv_rdo"][0]:
            groups.setdefault(c[1].tobytes(), []).append(k)
    return list(groups.values())


def test_search_pu_multi_batch(api):
    """kvz_hip_search_pu_multi_batch: every group of cases with one parameter record in one call, their plane pairs in the table behind a
    pair that belongs to no PU, the PUs interleaved by a seeded permutation"""
    fx = fixture()
    groups = multi_groups()
    assert sum(len(g) for g in groups) == sum(1 for c, _ in fx if not c[1]["mv_rdo"][0]) and max(len(g) for g in groups) >= 2
    for gi, group in enumerate(groups):
        decoy = fx[(group[0] + 1) % len(fx)][0]
        pics, refs, parts, wants, ctbs = [decoy[3]], [decoy[2]], [], [], []
        for j, k in enumerate(group):
            c, want = fx[k]
            pics.append(c[2]); refs.append(c[3])
            u = np.array(c[4])
            u["pad"] = ((j + 1) << 2) | (u["pad"] & 3)
            parts.append(u); wants.append(want); ctbs.append(c[6])
        order = np.random.default_rng(gi).permutation(sum(len(p) for p in parts))
        pus, want, ctb = np.concatenate(parts)[order], np.concatenate(wants)[order], np.concatenate(ctbs)[order]
        got = guarded("search_pu_multi_batch", lambda: launch(api, fx[group[0]][0][1], pics, refs, pus, None, ctb, multi=True))
        same(got, want, "multi batch of %s" % ", ".join(fx[k][0][0] for k in group))


def test_mv_rdo_cases_go_to_the_rdo_kernel(api):
    """the --mv-rdo cases again in one list per case with the snapshots shuffled: the kernel reads pus.reserved, not the position"""
    fx = [(c, w) for c, w in fixture() if c[1]["mv_rdo"][0]]
    assert len(fx) >= 6 and {int(c[1]["refs_before"][0]) for c, _ in fx} >= {1, 2, 4}
    for (name, prm, pic, ref, pus, cabac, ctb), want in fx:
        perm = np.random.default_rng(len(name)).permutation(len(cabac))
        u = np.array(pus)
        u["reserved"] = np.argsort(perm)[pus["reserved"]]
        same(guarded("search_pu_rdo_kernel", lambda: launch(api, prm, [pic], [ref], u, cabac[perm], ctb)), want, name + ": snapshots shuffled")


@pytest.mark.parametrize("qsad", [1, 0], ids=["qsad", "sad_u8"])
@pytest.mark.parametrize("workers", [0, 40], ids=["launches", "resident_workers"])
def test_search_service(api, workers, qsad):
    """every PU as a one-picture request to one service: the answer is the fixture's, under the case's cost to beat and, for the cases that
    set one, under 2147483647 too (the gate cases hold that PU a third time with a cost it beats).  full_qsad = 0: the exhaustive-search cases"""
    from kvazaar_amd import _lib
    L = _lib.load()
    fx = [(c, w) for c, w in fixture() if not c[1]["mv_rdo"][0] and (qsad or c[1]["algorithm"][0] == 3)]
    assert len(fx) >= 10
    for key, value in ((b"service_workers", workers), (b"full_qsad", qsad)):
        _lib.check(L.kvz_hip_set_tuning(key, value), "tuning")
    svc = guarded("service", lambda: api.MeService(192, 128, max_pictures=2, max_threads=4))
    try:
        req = np.zeros(1, dtype=ME_REQUEST)
        req["pic_slot"], req["n_refs"] = 0, 1
        req["ref_slot"][0, 0] = 1
        for (name, prm, pic, ref, pus, cabac, ctb), want in fx:
            guarded("service planes", lambda: (svc.put_plane(0, pic), svc.put_plane(1, ref)))
            p = np.array(prm)
            p["cost_to_beat"] = 0
            req["params"] = p[0]
            for i in range(len(pus)):
                req["pu"][0, 0] = pus[i]
                req["cost_to_beat"] = ctb[i]
                got = guarded("service search", lambda: svc.search(req))
                same(got, want[i:i + 1], "%s PU %d through the service" % (name, i))
                if name.startswith("gate-") and i % 3 == 0:              # (cost, cost - 1, cost + 1): the third is the open gate
                    req["cost_to_beat"] = MAX_INT
                    got = guarded("service search", lambda: svc.search(req))
                    same(got, want[i + 2:i + 3], "%s PU %d through the service, nothing to beat" % (name, i))
    finally:
        for key in (b"service_workers", b"full_qsad"):
            L.kvz_hip_set_tuning(key, -1)
        svc.close()

"""GPU: the transform-skip entries with the reference's pricing rule -- kvz_hip_inter_residual_frame_ts_cabac and
kvz_hip_intra_recon_frame_ts_cabac -- against tests/golden/trskip_cabac.npz (tests/trskip_cabac_cases.py: both trials from the reference's
own kvz_quantize_residual, the CABAC prices from its own counting coder, a set per LCU, a fast_limit per picture, one of them inside the
picture's QPs and one picture with lcu_ctx == NULL); every output the _ts tests compare, exactly.  With fast_limit above every QP, and
with pricing == NULL, the entries must reproduce the _ts entries byte for byte on the same inputs.  Every test runs under a time limit
of its own that ends the process, and after a call that reports a runtime error no further test starts anything on the device."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from lcu_qp_cases import zero_outputs
import trskip_cabac_cases as K
import trskip_cases as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PICS = {p[0]: p for p in T.FIXTURE_PICTURES}
TEST_LIMIT_S = 60
FAULTS = []


@pytest.fixture(autouse=True)
def limits():
    assert not FAULTS, "an earlier test met a device error (%s): nothing more is started" % FAULTS[0]
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def api():
    from kvazaar_amd import _lib, api as A
    _lib.init(0)
    return A


@pytest.fixture(scope="module")
def inputs():
    return np.load(os.path.join(HERE, "golden", "trskip.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "trskip_cabac.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lists():
    z = np.load(os.path.join(HERE, "golden", "scaling_list.npz"), allow_pickle=False)
    return z["default_quant"], z["default_dequant"]


def both(api, case, lists, pricing):
    """the two entries through the numpy wrappers, over zeroed outputs and a poisoned tr_skip map -> (mid, full); pricing None: the _ts entries"""
    chroma, w, h = case["chroma"], case["width"], case["height"]
    lq = case["lcu_qp"] if case["per_lcu"] else None
    tables = lists if case["lists"] else None
    poison = np.full(case["cus"].shape, T.POISON_SKIP, np.uint8)
    init = zero_outputs(w, h, chroma)
    try:
        mid = api.inter_residual_frame(case["src"], case["pred"], case["cus"], case["qp"], chroma, case["slice_is_intra"], case["signhide"], coeff=init[0],
                                       cbf_out=init[1], costs=init[2], lcu_qp=lq, scaling=tables, trskip=case["bit_cost"], tr_skip=poison, pricing=pricing)
        tiles = api.tile_grid(w, h, case["col_bd"], case["row_bd"]) if case["tiled"] else None
        full = api.intra_recon_frame(case["src"], mid["rec"], mid["cus"], case["modes"], case["qp"], chroma, case["signhide"], case["slice_is_intra"],
                                     coeff=mid["coeff"], cbf_out=mid["cbf_out"], costs=mid["costs"], lcu_qp=lq, tiles=tiles, scaling=tables,
                                     trskip=case["bit_cost"], tr_skip=mid["tr_skip"], pricing=pricing)
    except Exception:
        FAULTS.append("a _ts_cabac call")
        raise
    return mid, full


def pricing_of(api, case, fast_limit=None):
    return dict(sets=K.records(api), fast_limit=K.PRICING[case["name"]][0] if fast_limit is None else fast_limit, lcu_ctx=K.lcu_ctx_of(case))


@pytest.mark.parametrize("name", list(PICS))
def test_fixture_through_both_entries(api, inputs, golden, lists, name):
    case = T.load_case(inputs, PICS[name])
    chroma = case["chroma"]
    assert (K.lcu_ctx_of(case) is None) == (name == "inter")
    mid, full = both(api, case, lists, pricing_of(api, case))
    T.assert_outputs_equal(mid, T.load_want(golden, name, "mid", chroma), "%s inter" % name, chroma)
    T.assert_outputs_equal(full, T.load_want(golden, name, "full", chroma), "%s intra" % name, chroma)
    # the fixture tells the pricing rules apart: the _ts fixture holds other choices
    dec = golden[name + "_decided"]
    assert (dec[:, 3] != dec[:, 4]).sum() >= K.MIN_DIFFERENT
    assert (T.load_want(golden, name, "full", chroma)["tr_skip"] != T.load_want(inputs, name, "full", chroma)["tr_skip"]).any()


def test_the_limit_straddles_the_qps_of_mixed(inputs, golden):
    case = T.load_case(inputs, PICS["mixed"])
    qps = set(int(q) for q in case["lcu_qp"])
    limit = K.PRICING["mixed"][0]
    assert min(qps) < limit <= max(qps)
    dec = golden["mixed_decided"]
    assert 0 < dec[:, 5].sum() < len(dec) and (dec[dec[:, 5] == 0][:, 3] == dec[dec[:, 5] == 0][:, 4]).all()
    assert max(K.lcu_ctx_of(case)) >= K.N_SETS                  # an index beyond the table, used as the last set


@pytest.mark.parametrize("name", list(PICS))
def test_limit_above_every_qp_and_null_pricing_are_the_ts_entries(api, inputs, lists, name):
    case = T.load_case(inputs, PICS[name])
    chroma = case["chroma"]
    ts_mid, ts_full = both(api, case, lists, None)
    T.assert_outputs_equal(ts_full, T.load_want(inputs, name, "full", chroma), "%s: the _ts entries" % name, chroma)
    for what, pricing in (("fast_limit 52", pricing_of(api, case, fast_limit=52)), ("pricing == NULL", {})):
        mid, full = both(api, case, lists, pricing)
        T.assert_outputs_equal(mid, ts_mid, "%s inter, %s" % (name, what), chroma)
        T.assert_outputs_equal(full, ts_full, "%s intra, %s" % (name, what), chroma)


def test_the_entries_refuse_and_delegate_on_a_device(api):
    """the error paths and the pricing == NULL / ts == NULL delegation of tests/test_coeff_cost_abi.py, here where a device answers"""
    import test_coeff_cost_abi as CA
    CA.test_the_stages_refuse_and_delegate()
    CA.test_every_error_path_returns_invalid_or_no_device()

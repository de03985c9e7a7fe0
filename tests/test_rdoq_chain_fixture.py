"""CPU: tests/golden/rdoq_chain.npz -- what kvz_hip_inter_residual_frame_rdoq and kvz_hip_intra_recon_frame_rdoq must leave (tests/rdoq_chain_cases.py).
Where the reference is compiled the fixture is regenerated from its own kvz_quantize_residual under cfg.rdoq_enable and compared with the
committed file, array by array, byte for byte, and the generator's conditions are asserted.  Everywhere, the fixture is recomposed without
the reference -- levels from tests/rdoq_model.py, transforms and dequantisation from the oracle -- and must come out the same; and every
deliberate error of rdoq_chain_cases.MUTANTS must change at least one stored byte, or the fixture could not tell that error from the
entries."""
import os

import numpy as np
import pytest

import inter_residual_cases as RC
import rdoq_chain_cases as K
import ref_quant_rdoq as Q

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rdoq_chain.npz")


def _npz(name):
    return np.load(os.path.join(HERE, "golden", name), allow_pickle=False)


@pytest.fixture(scope="module")
def model():
    """the model's composition of every picture, computed once: {name: (case, mid, full)}, and the cache of levels the mutants share"""
    inputs, golden = _npz("lcu_qp.npz"), _npz("rdoq_chain.npz")
    tables = K.model_tables(_npz("rdoq.npz"), _npz("scaling_list.npz"))
    cache, out = {}, {}
    for pic in K.PICTURES:
        name, w, h, chroma, signhide, slice_is_intra = pic
        case = K.load_inputs(inputs, pic, golden)
        out[name] = (case,) + K.compose_chain(name, case, K.Model(tables, cache=cache), chroma, signhide, slice_is_intra)
    return {"tables": tables, "cache": cache, "pictures": out, "golden": golden}


def test_file_is_small_and_holds_outputs_and_own_inputs_only():
    z = _npz("rdoq_chain.npz")
    assert os.path.getsize(GOLDEN) < 350 * 1000
    for key in z.files:
        name, kind = key.split("_", 1)
        assert name in K.SETTINGS and (kind.split("_")[0] in ("mid", "full", "tiled") or (kind.startswith("in_") and name in K.OWN_INPUTS)), key
    # the stored inputs are what the module makes
    for pic in K.PICTURES:
        if pic[0] in K.OWN_INPUTS:
            made, stored = K.own_inputs(pic), K.load_inputs(None, pic, z)
            for a, b in zip(made, stored):
                for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                    assert (u is None and v is None) or np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)), pic[0]


def test_settings_are_what_the_issue_asks():
    ranges, dumps, lambdas = K.context_sets()
    assert len(dumps) == K.N_SETS == 6 and dumps.max() <= 125 and (lambdas > 0).all() and len(set(lambdas.tolist())) == 6
    assert K.lcu_ctx_of("mono", 96, 72) is None and K.SETTINGS["mono"][0] == 1 and K.SETTINGS["ragged"][0] == 0
    assert K.SETTINGS["coarse"] == (0, True, 1)
    ctx = K.lcu_ctx_of("ragged", 200, 136)
    assert ctx.max() >= K.N_SETS and len(set(np.minimum(ctx, K.N_SETS - 1).tolist())) >= 4
    assert K.rdoq_cases.lambda_of(K.SET_LAMBDA_QP[4]) == lambdas[4] and K.SET_LAMBDA_QP[4] == 12


@pytest.mark.parametrize("name", [p[0] for p in K.PICTURES])
def test_model_composition_equals_the_fixture(model, name):
    chroma = dict((p[0], p[3]) for p in K.PICTURES)[name]
    case, mid, full = model["pictures"][name]
    RC.assert_outputs_equal(mid, K.load_want(model["golden"], name + "_mid", chroma), name + " after the inter stage", chroma)
    RC.assert_outputs_equal(full, K.load_want(model["golden"], name + "_full", chroma), name + " after the intra stage", chroma)


def test_model_composition_of_the_tiled_run_equals_the_fixture(model):
    pic = K.PICTURES[0]
    name, w, h, chroma, signhide, slice_is_intra = pic
    assert name == "ragged" and name in K.TILE_GRID
    case = model["pictures"][name][0]
    _, tiled = K.compose_chain(name, case, K.Model(model["tables"], cache=model["cache"]), chroma, signhide, slice_is_intra, grid=K.TILE_GRID[name])
    RC.assert_outputs_equal(tiled, K.load_want(model["golden"], name + "_tiled", chroma), "ragged tiled", chroma)


def _stored_bytes(mid, full, chroma):
    out = []
    for o in (mid, full):
        out += [np.asarray(p) for p in o["rec"][:3 if chroma else 1]] + [np.asarray(c) for c in o["coeff"][:3 if chroma else 1]]
        out += [o["cus"].view(np.uint8), o["cbf_out"], o["costs"].view(np.uint32)]
    return out


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_deliberate_error_changes_a_stored_byte(model, mutant):
    changed = []
    for pic in K.PICTURES:
        name, w, h, chroma, signhide, slice_is_intra = pic
        case, mid, full = model["pictures"][name]
        mid2, full2 = K.compose_chain(name, case, K.Model(model["tables"], mutant=mutant, cache=model["cache"]), chroma, signhide, slice_is_intra)
        if any((a != b).any() for a, b in zip(_stored_bytes(mid, full, chroma), _stored_bytes(mid2, full2, chroma))):
            changed.append(name)
    assert changed, mutant
    # the errors that only one picture can show, where the issue names the picture
    if mutant == "rdoq-on-skipped-4x4":
        assert changed == ["mono"]
    if mutant == "tr-depth-of-the-cus-first-record":
        assert changed == ["deep"]


@pytest.mark.skipif(not Q.available(), reason="compiled reference not built")
def test_fixture_regenerates_from_the_compiled_reference_byte_for_byte():
    import gen_rdoq_chain_golden as G
    d, missing = G.build()
    assert not missing, missing
    z = _npz("rdoq_chain.npz")
    assert sorted(d) == sorted(z.files)
    for key in z.files:
        a, b = np.ascontiguousarray(d[key]), z[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key

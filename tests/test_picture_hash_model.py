"""CPU: the numpy model of the picture hash (tests/picture_hash_model.py) against the compiled reference's array_checksum -- generic,
generic4 and generic8, reached in a child process through the exported kvz_strategy_register_nal on the harness's list, and the
function behind the reference's own kvz_array_checksum -- on every case of tests/picture_hash_cases.py; the committed golden against
the same; and every deliberate error of the model noticed by at least one case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import picture_hash_cases as HC
import picture_hash_model as M
import ref_lib as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "picture_hash.npz")

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def model():
    """the model's values in the golden's layout, computed once"""
    planes = [M.plane_checksum(*HC.plane(p[0])) for p in HC.PLANES + (HC.WRAP,)]
    pictures = [M.picture(*HC.picture(p[0]))[1] for p in HC.PICTURES + (HC.EXTREME,)]
    return {"planes": planes, "pictures": [[int(v) for v in p["checksum"]] for p in pictures], "sse": [[int(v) for v in p["sse"]] for p in pictures]}


@pytest.fixture(scope="module")
def reference():
    """a child process: registering the nal group changes the harness's list"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "gen_picture_hash_golden.py"), "--dump"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@needs_ref
@pytest.mark.parametrize("name", ("generic", "generic4", "generic8", "selected"))
def test_model_equals_the_reference_on_every_case(reference, model, name):
    assert reference[name]["planes"] == model["planes"]
    assert reference[name]["pictures"] == model["pictures"]


@needs_ref
def test_golden_holds_the_reference_results(reference, golden):
    from gen_picture_hash_golden import squared_errors
    assert golden["plane_checksum"].tolist() == reference["generic"]["planes"]
    assert golden["picture_checksum"].tolist() == reference["generic"]["pictures"]
    assert golden["sao_dst_checksum"].tolist() == reference["generic"]["sao"]
    pictures, sao = squared_errors()
    assert golden["picture_sse"].tolist() == pictures and golden["sao_dst_sse"].tolist() == sao


def test_model_equals_the_golden(model, golden):
    assert golden["plane_checksum"].tolist() == model["planes"]
    assert golden["picture_checksum"].tolist() == model["pictures"]
    assert golden["picture_sse"].tolist() == model["sse"]
    assert golden["plane_checksum"][-1] == HC.WRAP_CHECKSUM == (255 * 4352 * 4096) % 2 ** 32
    extreme = golden["picture_sse"][-1]
    assert extreme[0] == 520 * 520 * 255 ** 2 and int(extreme.sum()) > 1.75e10 and extreme[0] >= 2 ** 32


def test_lcu_records_add_up_to_the_planes():
    for p in HC.PICTURES + (HC.EXTREME,):
        rec, src, w, h, chroma = HC.picture(p[0])
        lcus, pic = M.picture(rec, src, w, h, chroma)
        assert pic["n_lcu"] == len(lcus) == ((w + 63) // 64) * ((h + 63) // 64)
        for c in range(3):
            if c and not chroma:
                assert not lcus["checksum"][:, c].any() and not lcus["sse"][:, c].any() and pic["checksum"][c] == 0 and pic["sse"][c] == 0
                continue
            pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
            assert int(lcus["checksum"][:, c].astype(np.uint64).sum()) % 2 ** 32 == pic["checksum"][c] == M.plane_checksum(rec[c], pw, ph)
            assert int(lcus["sse"][:, c].astype(np.uint64).sum()) == pic["sse"][c] == M.plane_sse(src[c], rec[c], pw, ph)
        assert (M.picture(rec, None, w, h, chroma)[1]["sse"] == 0).all()


def test_sei_bytes_are_big_endian():
    assert M.RULE.sei_bytes(0x01020304) == b"\x01\x02\x03\x04"


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_deliberate_error_is_noticed(model, fault):
    """the cases are worth something only if a wrong rule fails on them: each fault changes at least one value that the tests compare"""
    bad = M.Rule(fault)
    if fault == "little_endian":
        assert any(bad.sei_bytes(v) != M.RULE.sei_bytes(v) for v in model["planes"])
        return
    if fault in ("luma_coords_for_chroma", "sse_in_32_bits", "chroma_rounded_up"):
        # picture-level faults.  Picture sizes are multiples of 8, where rounding the chroma size up changes nothing: that one is
        # looked for on an odd picture, 13 x 7, which only the model takes
        if fault == "chroma_rounded_up":
            g = np.random.default_rng(77)
            rec = tuple(g.integers(0, 256, (7 + HC.PAD_ROWS, 29), dtype=np.uint8) for _ in range(3))
            got, want = bad.picture(rec, None, 13, 7, 1)[1], M.picture(rec, None, 13, 7, 1)[1]
            assert (got["checksum"] != want["checksum"]).any()
            return
        names = [p[0] for p in HC.PICTURES + (HC.EXTREME,)]
        pics = [bad.picture(*HC.picture(n))[1] for n in names]
        assert [[int(v) for v in p["checksum"]] for p in pics] != model["pictures"] or [[int(v) for v in p["sse"]] for p in pics] != model["sse"]
        return
    # the planes in their order, the large wrap plane last and only if nothing before it noticed
    assert any(bad.plane_checksum(*HC.plane(p[0])) != want for p, want in zip(HC.PLANES + (HC.WRAP,), model["planes"])), fault

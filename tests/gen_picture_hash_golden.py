"""Writes tests/golden/picture_hash.npz: what the compiled reference's array_checksum gives for the planes and pictures of
tests/picture_hash_cases.py and for the dst planes of tests/golden/sao_frame.npz, with the squared errors beside them.  Values only:
the inputs are regenerated from seeds.  Needs the compiled reference (oracle/_ref).

The reference's nal group is not in the harness's list, so reference_results() registers it there itself, with the exported
kvz_strategy_register_nal on ref_list(), and reaches generic, generic4 and generic8 through ref_strategy.  That changes the list, so
callers run it in a process of its own: `python gen_picture_hash_golden.py --dump` prints the results as JSON
(tests/test_picture_hash_model.py reads them that way).

The squared error has no function in the reference's library (compute_psnr is a static function of its command-line tool,
encmain.c:101-129, a double sum of (src - rec)^2 that is exact below 2^53): the golden holds the same sum in int64."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import picture_hash_cases as HC  # noqa: E402
import picture_hash_model as M  # noqa: E402
import ref_lib as R  # noqa: E402

NAMES = ("generic", "generic4", "generic8")
GOLDEN = os.path.join(HERE, "golden", "picture_hash.npz")
SAO_GOLDEN = os.path.join(HERE, "golden", "sao_frame.npz")
CHECKSUM_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_uint8)      # strategies-nal.h:34-39


def reference_functions():
    """{name: array_checksum of that name}, plus "selected": the function behind the reference's own kvz_array_checksum"""
    L = R.lib()
    L.kvz_strategy_register_nal.restype = C.c_int
    L.kvz_strategy_register_nal.argtypes = [C.c_void_p, C.c_uint8]
    if not L.ref_strategy(b"array_checksum", b"generic"):
        assert L.kvz_strategy_register_nal(L.ref_list(), 8)
    fns = {n: CHECKSUM_FN(L.ref_strategy(b"array_checksum", n.encode())) for n in NAMES}
    fns["selected"] = CHECKSUM_FN(C.c_void_p.in_dll(L, "kvz_array_checksum").value)
    return fns


def call(fn, buf, width, height):
    """-> the checksum that fn leaves as four big-endian bytes; the other twelve bytes of the SEI array must stay as they were"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    out = (C.c_ubyte * 16)(*([0xEE] * 16))
    fn(buf.ctypes.data, height, width, buf.shape[1], out, 8)
    assert bytes(out[4:]) == b"\xEE" * 12
    return int.from_bytes(bytes(out[:4]), "big")


def sao_fixture_planes():
    """[(name, chroma, src planes, dst planes)] of the committed SAO-frame fixture"""
    z = np.load(SAO_GOLDEN, allow_pickle=False)
    out = []
    for name, chroma in HC.SAO_FIXTURE:
        pick = lambda kind: tuple(z["%s_%s_%s" % (name, kind, n)] if (n == "y" or chroma) else None for n in "yuv")
        out.append((name, chroma, pick("src"), pick("dst")))
    return out


def reference_results():
    """every value of the golden, per reference function: {name: {"planes": [...], "pictures": [[y, u, v]], "sao": [[y, u, v]]}}"""
    fns = reference_functions()
    res = {}
    for n, fn in fns.items():
        planes = [call(fn, *HC.plane(p[0])) for p in HC.PLANES + (HC.WRAP,)]
        pictures = []
        for p in HC.PICTURES + (HC.EXTREME,):
            rec, _, w, h, chroma = HC.picture(p[0])
            pictures.append([call(fn, rec[k], w >> (1 if k else 0), h >> (1 if k else 0)) if (k == 0 or chroma) else 0 for k in range(3)])
        sao = [[call(fn, dst[k], dst[k].shape[1], dst[k].shape[0]) if (k == 0 or chroma) else 0 for k in range(3)]
               for (_, chroma, _, dst) in sao_fixture_planes()]
        res[n] = {"planes": planes, "pictures": pictures, "sao": sao}
    return res


def squared_errors():
    pictures = []
    for p in HC.PICTURES + (HC.EXTREME,):
        rec, src, w, h, chroma = HC.picture(p[0])
        pictures.append([M.plane_sse(src[k], rec[k], w >> (1 if k else 0), h >> (1 if k else 0)) if (k == 0 or chroma) else 0 for k in range(3)])
    sao = [[M.plane_sse(src[k], dst[k], dst[k].shape[1], dst[k].shape[0]) if (k == 0 or chroma) else 0 for k in range(3)]
           for (_, chroma, src, dst) in sao_fixture_planes()]
    return pictures, sao


if __name__ == "__main__":
    assert R.available(), "the golden is written from the compiled reference only"
    res = reference_results()
    if "--dump" in sys.argv:
        print(json.dumps(res))
        sys.exit(0)
    assert all(res[n] == res["generic"] for n in res), "the reference's functions disagree"
    sse_pictures, sse_sao = squared_errors()
    np.savez_compressed(GOLDEN, plane_checksum=np.array(res["generic"]["planes"], np.uint32),
                        picture_checksum=np.array(res["generic"]["pictures"], np.uint32), picture_sse=np.array(sse_pictures, np.uint64),
                        sao_dst_checksum=np.array(res["generic"]["sao"], np.uint32), sao_dst_sse=np.array(sse_sao, np.uint64))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")

"""CPU: the declarations of the two lossless entries: declared, documented, exported with the kvz_ prefix and bound; kvz_hip_lossless in
C and ctypes; the header no longer calls lossless coding out of scope for the residual stages; without a device the entries refuse."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import test_abi as A

ENTRIES = ("kvz_hip_inter_residual_frame_lossless", "kvz_hip_intra_recon_frame_lossless")


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    for name in ENTRIES:
        assert name.startswith("kvz_") and name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
        assert re.search(r"\bT %s\b" % name, exported), name
        res, args = B.SIGNATURES[name]
        params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1).split(",")]
        assert res is ctypes.c_int and len(args) == len(params), name
        assert params[-2:] == ["const kvz_hip_lossless *ll", "kvz_hip_stream s"] and args[-2] == ctypes.POINTER(B.Lossless), name
    # the lossy entries' signatures without params, lcu_qp, tables and transform skip
    old = [p.strip() for p in re.search(r"KVZ_HIP_API int kvz_hip_inter_residual_frame\(([^;]*)\);", src).group(1).split(",")]
    new = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % ENTRIES[0], src).group(1).split(",")]
    assert new[:-2] == old[:-2]
    old = [p.strip() for p in re.search(r"KVZ_HIP_API int kvz_hip_intra_recon_frame_tiles\(([^;]*)\);", src).group(1).split(",")]
    new = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % ENTRIES[1], src).group(1).split(",")]
    assert new[:-3] == old[:-4] and new[-3] == "const kvz_hip_tile_grid *tiles"


def test_struct_in_c_and_ctypes(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu %d\\n", sizeof(kvz_hip_lossless), offsetof(kvz_hip_lossless, chroma), offsetof(kvz_hip_lossless, implicit_rdpcm),'
             ' offsetof(kvz_hip_lossless, reserved), KVZ_HIP_ABI_VERSION);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [16, 0, 4, 8, 4]
    assert ctypes.sizeof(B.Lossless) == 16 and [getattr(B.Lossless, f).offset for f in ("chroma", "implicit_rdpcm", "reserved")] == [0, 4, 8]


def test_header_documents_the_entries():
    text = open(A.HEADER).read()
    doc = text[text.index("Lossless coding in the picture chain"):text.index("KVZ_HIP_API int " + ENTRIES[1])]
    for what in ("TAKEN\n *   FROM THE SOURCE PLANE", "encoderstate.c:1125-1127", "ONE kernel launch", "intra.c:621", "transform.c:109-123", "transform.c:315-316",
                 "search.c:580", "encoder.c:623-628", "search_intra.c:419", "PCM", "bit depths above 8", "KVZ_HIP_ERR_INVALID", "STORED value non-zero"):
        assert what in doc, what
    # lossless coding is no longer out of scope for the two residual stages, their _sl and their _ts entries
    for m in re.finditer(r"OUT OF SCOPE[^/]*?\*/", text, flags=re.S):
        scope = m.group(0)
        if "kvz_filter_deblock_lcu" in scope:
            continue
        assert "lossless coding" not in scope.split("Lossless coding has")[0].replace("Lossless coding switches", ""), scope[:200]
    assert text.count("kvz_hip_inter_residual_frame_lossless") >= 5 and text.count("kvz_hip_intra_recon_frame_lossless") >= 5


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    p = inspect.signature(api.inter_residual_frame_lossless).parameters
    assert list(p) == ["src", "pred", "cus", "chroma", "implicit_rdpcm", "coeff", "cbf_out", "costs"]
    assert p["chroma"].default == 1 and p["implicit_rdpcm"].default == 0 and p["coeff"].default is None
    p = inspect.signature(api.intra_recon_frame_lossless).parameters
    assert list(p) == ["src", "rec", "cus", "modes", "chroma", "implicit_rdpcm", "tiles", "coeff", "cbf_out", "costs"]
    assert p["tiles"].default is None and p["implicit_rdpcm"].default == 0
    # next to _residual_frame, not threaded through it
    assert "lossless" not in inspect.signature(api._residual_frame).parameters and "implicit_rdpcm" not in inspect.signature(api._residual_frame).parameters


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_argument_checks_return_invalid_or_no_device():
    """with a device every NULL is refused as invalid; without one the entries say so before they look at anything"""
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    want = invalid if torch.cuda.is_available() else no_device
    for name in ENTRIES:
        args = [0 if t is ctypes.c_uint32 else None for t in B.SIGNATURES[name][1]]
        assert getattr(L, name)(*args) == want, name
        ll = B.Lossless(1, 0, (0, 7))
        args[-2] = ctypes.byref(ll)
        assert getattr(L, name)(*args) == want, name

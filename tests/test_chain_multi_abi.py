"""CPU: the declarations of the two multi-picture entries of the picture chain: declared, documented, exported with the kvz_ prefix and
bound; kvz_hip_chain_picture in C and ctypes; the limit of sixteen pictures; the ABI version; the numpy conveniences; without a device
the entries refuse before they look at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRIES = ("kvz_hip_inter_residual_frames", "kvz_hip_intra_recon_frames")
FIELDS = ("src", "rec_y", "rec_u", "rec_v", "stride_y", "stride_c", "cus", "intra_modes", "coeff_y", "coeff_u", "coeff_v", "cbf_out", "costs",
          "lcu_qp", "params")
OFFSETS = [0, 40, 48, 56, 64, 68, 72, 80, 88, 96, 104, 112, 120, 128, 136]


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
        assert params == ["const kvz_hip_chain_picture *pictures", "int n_pictures", "kvz_hip_stream s"], name
        assert res is ctypes.c_int and args == [ctypes.POINTER(B.ChainPicture), ctypes.c_int, ctypes.c_void_p], name


def test_struct_in_c_and_ctypes(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d", sizeof(kvz_hip_chain_picture), KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_chain_picture, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [160, 16, 4] + OFFSETS
    assert ctypes.sizeof(B.ChainPicture) == 160 and [getattr(B.ChainPicture, f).offset for f in FIELDS] == OFFSETS
    assert [f for f, _ in B.ChainPicture._fields_] == list(FIELDS)
    assert ctypes.sizeof(B.RefPicture) == 40 and ctypes.sizeof(B.InterResidualParams) == 24
    assert B.MAX_CHAIN_PICTURES == 16
    # the header states what the compiler says
    text = open(A.HEADER).read()
    decl = text[text.index("#define KVZ_HIP_MAX_CHAIN_PICTURES 16"):text.index("} kvz_hip_chain_picture;")]
    for f, off in zip(FIELDS, OFFSETS):
        assert re.search(r"[ *]%s[;,][^\n]*/\*[^\n]*\b%d\b" % (f, off), decl), (f, off)
    assert "kvz_hip_chain_picture;                /* 160 bytes */" in text


def test_header_documents_the_entries():
    text = open(A.HEADER).read()
    doc = text[text.index("Several independent pictures through the residual stages at once"):text.index("KVZ_HIP_API int " + ENTRIES[0])]
    for what in ("THE RULE", "byte for byte", "kvz_hip_inter_residual_frame_qp", "kvz_hip_intra_recon_frame_qp", "lcu_qp == NULL", "Independence is the caller's promise",
                 "rec_y, cus or coeff_y base pointers coincide", "n_pictures == 0 is a no-op", "KVZ_HIP_ERR_INVALID", "nothing is written for any picture",
                 "names the\n *   index of the offending record", "no host synchronisation, no allocation, no workspace", "kvz_hip_graph_begin",
                 "ceil(width / 64) + 2 (ceil(height / 64) - 1)", "LEFT OUT ON PURPOSE", "tiles, scaling lists or transform skip", "--lossless",
                 "the QP map, deblocking and SAO", "4:0:0 next to 4:2:0", "The ABI version stays 4"):
        assert what in doc, what


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    for f in (api.inter_residual_frames, api.intra_recon_frames):
        assert list(inspect.signature(f).parameters) == ["pictures"]
    assert api.MAX_CHAIN_PICTURES == 16
    # next to the single-picture conveniences, not threaded through them
    assert "pictures" not in inspect.signature(api._residual_frame).parameters
    assert "_chain_frames" not in inspect.getsource(api._residual_frame) and "_residual_frame(" not in inspect.getsource(api._chain_frames)


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_argument_checks_return_invalid_or_no_device():
    """with a device NULL records and a count outside 0..16 are refused as invalid; without one the entries say so before they look at
    anything"""
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    records = (B.ChainPicture * 17)()
    for name in ENTRIES:
        f = getattr(L, name)
        assert f(None, 1, None) == want, name
        assert f(records, 17, None) == want and f(records, -1, None) == want, name
        assert f(records, 1, None) == want, name                          # a record of NULL pointers
        assert f(None, 0, None) == (0 if have else no_device), name

"""CPU: the declarations of the two multi-picture entries that take tiles, scaling lists and transform skip: declared, documented, exported
with the kvz_ prefix and bound; kvz_hip_chain_picture_ts in C and ctypes; the capacity of the pool of tile boundaries; kvz_hip_chain_picture
and the ABI version unchanged; the numpy conveniences; without a device the entries refuse before they look at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRIES = ("kvz_hip_inter_residual_frames_ts", "kvz_hip_intra_recon_frames_ts")
FIELDS = ("pic", "grid", "tables", "ts", "tr_skip_out")
OFFSETS = [0, 160, 168, 184, 192]


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
        assert params == ["const kvz_hip_chain_picture_ts *pictures", "int n_pictures", "kvz_hip_stream s"], name
        assert res is ctypes.c_int and args == [ctypes.POINTER(B.ChainPictureTs), ctypes.c_int, ctypes.c_void_p], name


def test_struct_in_c_and_ctypes(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %d %d %d", sizeof(kvz_hip_chain_picture_ts), sizeof(kvz_hip_chain_picture), KVZ_HIP_CHAIN_TILE_BOUNDS,',
             '         KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_chain_picture_ts, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:2] == [200, 160] and got[3:] == [16, 4] + OFFSETS
    assert got[2] >= 256 and got[2] == B.CHAIN_TILE_BOUNDS
    assert ctypes.sizeof(B.ChainPictureTs) == 200 and [getattr(B.ChainPictureTs, f).offset for f in FIELDS] == OFFSETS
    assert [f for f, _ in B.ChainPictureTs._fields_] == list(FIELDS)
    assert ctypes.sizeof(B.ChainPicture) == 160 and ctypes.sizeof(B.ScalingTables) == 16 and ctypes.sizeof(B.TrSkip) == 16
    # the header states what the compiler says
    text = open(A.HEADER).read()
    decl = text[text.index("#define KVZ_HIP_CHAIN_TILE_BOUNDS"):text.index("} kvz_hip_chain_picture_ts;")]
    for f, off in zip(FIELDS, OFFSETS):
        assert re.search(r"[ *]%s;[^\n]*/\*\s*%d:" % (f, off), decl), (f, off)
    assert "kvz_hip_chain_picture_ts;         /* 200 bytes */" in text
    assert "kvz_hip_chain_picture;                /* 160 bytes */" in text


def test_header_documents_the_entries():
    text = open(A.HEADER).read()
    doc = text[text.index("} kvz_hip_chain_picture_ts;"):text.index("KVZ_HIP_API int " + ENTRIES[0])]
    for what in ("THE RULE", "byte for byte", "kvz_hip_inter_residual_frame_ts", "kvz_hip_intra_recon_frame_ts", "ONE RESTRICTION", "homogeneous",
                 "differs from record 0", "grid == NULL", "No options at all", "kvz_hip_inter_residual_frames", "tr_skip_out base", "KVZ_HIP_ERR_INVALID",
                 "writes nothing for any picture", "names the record's index", "KVZ_HIP_CHAIN_TILE_BOUNDS", "at which it overflowed",
                 "no host synchronisation, no allocation, no workspace", "kvz_hip_graph_begin", "w_t + 2 (h_t - 1)", "LEFT OUT ON PURPOSE", "--lossless",
                 "The ABI version stays 4"):
        assert what in doc, what


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    for f in (api.inter_residual_frames_ts, api.intra_recon_frames_ts):
        assert list(inspect.signature(f).parameters) == ["pictures"]
    assert api.CHAIN_TILE_BOUNDS >= 256 and api.MAX_CHAIN_PICTURES == 16
    for key in ("grid", "tables", "trskip"):
        assert key in inspect.signature(api._ChainPictureTs.__init__).parameters
    # next to the plain multi-picture conveniences, not threaded through them
    assert "_ts" not in inspect.getsource(api._chain_frames)


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
    records = (B.ChainPictureTs * 17)()
    for name in ENTRIES:
        f = getattr(L, name)
        assert f(None, 1, None) == want, name
        assert f(records, 17, None) == want and f(records, -1, None) == want, name
        assert f(records, 1, None) == want, name                          # a record of NULL pointers
        assert f(None, 0, None) == (0 if have else no_device), name

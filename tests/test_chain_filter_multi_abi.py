"""CPU: the declarations of the four multi-picture entries behind the residual stages -- the QP map, deblocking, the SAO statistics and
SAO of several pictures: declared, documented, exported with the kvz_ prefix and bound; kvz_hip_filter_picture in C99 and ctypes and in
the header's comments; the pool of tile boundaries and the ABI version unchanged; the numpy conveniences; without a device the entries
refuse before they look at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRIES = ("kvz_hip_cu_qp_frames", "kvz_hip_deblock_frames", "kvz_hip_sao_stats_frames", "kvz_hip_sao_frames")
FIELDS = ("width", "height", "chroma", "reserved", "src", "rec_y", "rec_u", "rec_v", "stride_y", "stride_c", "dst_y", "dst_u", "dst_v", "dst_stride_y",
          "dst_stride_c", "cus", "cbf", "lcu_qp", "lcu_last_qp", "stats", "cands", "sao_luma", "sao_chroma", "grid", "deblock", "cu_qp")
OFFSETS = [0, 4, 8, 12, 16, 56, 64, 72, 80, 84, 88, 96, 104, 112, 116, 120, 128, 136, 144, 152, 160, 168, 176, 184, 192, 256]
SIZE = 264


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
        assert params == ["const kvz_hip_filter_picture *pictures", "int n_pictures", "kvz_hip_stream s"], name
        assert res is ctypes.c_int and args == [ctypes.POINTER(B.FilterPicture), ctypes.c_int, ctypes.c_void_p], name


def test_struct_in_c99_and_ctypes_and_in_the_header_comments(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d", sizeof(kvz_hip_filter_picture), KVZ_HIP_CHAIN_TILE_BOUNDS, KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_filter_picture, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [SIZE, B.CHAIN_TILE_BOUNDS, 16, 4] + OFFSETS
    assert ctypes.sizeof(B.FilterPicture) == SIZE and [getattr(B.FilterPicture, f).offset for f in FIELDS] == OFFSETS
    assert [f for f, _ in B.FilterPicture._fields_] == list(FIELDS)
    assert ctypes.sizeof(B.DeblockParams) == 64 and ctypes.sizeof(B.CuQpTilesParams) == 8 and ctypes.sizeof(B.RefPicture) == 40
    # no implicit padding: the fields fill the record
    sizes = [getattr(B.FilterPicture, f).size for f in FIELDS]
    assert [o + s for o, s in zip(OFFSETS, sizes)] == OFFSETS[1:] + [SIZE]
    # the header states what the compiler says
    text = open(A.HEADER).read()
    decl = text[text.index("One picture of kvz_hip_cu_qp_frames"):text.index("} kvz_hip_filter_picture;")]
    decl = decl[decl.index("typedef struct {"):]
    stated = {}
    for line in decl.splitlines():
        m = re.match(r"\s*(?:const )?[\w ]+?[ *]([\w, *]+);\s*/\*\s*([\d, ]+):", line)
        if m:
            names = [n.strip(" *") for n in m.group(1).split(",")]
            offs = [int(v) for v in m.group(2).split(",")]
            assert len(offs) == len(names), line
            stated.update(zip(names, offs))
    assert stated == dict(zip(FIELDS, OFFSETS))
    assert "} kvz_hip_filter_picture;               /* 264 bytes */" in text


def test_header_documents_the_entries():
    text = open(A.HEADER).read()
    doc = text[text.index("} kvz_hip_filter_picture;"):text.index("KVZ_HIP_API int " + ENTRIES[0])]
    for what in ("THE RULE", "byte for byte", "kvz_hip_cu_qp_frame_tiles", "kvz_hip_deblock_frame_tiles", "kvz_hip_sao_frame_tiles", "kvz_hip_sao_stats_frame",
                 "grid == NULL", "chain_lcus = 0", "ceil(width / 64)", "no homogeneity rule", "4:0:0 beside 4:2:0", "tiled beside untiled",
                 "output base pointers coincide", "inputs may be shared", "n_pictures == 0 is a no-op", "KVZ_HIP_ERR_INVALID", "deblock.chroma != chroma",
                 "dst == rec", "writes nothing", "picture 2", "KVZ_HIP_CHAIN_TILE_BOUNDS", "at which it", "no host synchronisation, no allocation, no workspace",
                 "no atomics", "scalar loads", "below 4 KB", "kvz_hip_graph_begin", "presence of cands", "3 for kvz_hip_cu_qp_frames",
                 "2 for kvz_hip_deblock_frames", "LEFT OUT ON PURPOSE", "kvz_hip_inter_recon_frame", "--lossless", "The ABI version stays 4"):
        assert what in doc, what
    # both older multi-picture sections point here and no longer call these stages follow-ups
    for older in ("KVZ_HIP_API int kvz_hip_inter_residual_frames(", "KVZ_HIP_API int kvz_hip_inter_residual_frames_ts("):
        before = text[:text.index(older)]
        tail = before[before.rindex("LEFT OUT ON PURPOSE"):]
        assert "kvz_hip_cu_qp_frames" in tail and "kvz_hip_sao_frames" in tail and "follow-ups" not in tail


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    for f in (api.cu_qp_frames, api.deblock_frames, api.sao_stats_frames, api.sao_frames):
        assert list(inspect.signature(f).parameters) == ["pictures"]
    for name, keys in (("cu_qp", ("cus", "cbf", "lcu_qp", "start_qp", "tiles", "chain_rows")), ("deblock", ("y", "u", "v", "cus", "prm", "tiles")),
                       ("sao_stats", ("src", "rec", "chroma", "with_cands")), ("sao", ("rec", "sao_luma", "sao_chroma", "chroma", "dst", "tiles"))):
        assert list(inspect.signature(getattr(api._FilterPicture, name)).parameters) == list(keys)


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
    records = (B.FilterPicture * 17)()
    for name in ENTRIES:
        f = getattr(L, name)
        assert f(None, 1, None) == want, name
        assert f(records, 17, None) == want and f(records, -1, None) == want, name
        assert f(records, 1, None) == want, name                          # a record of NULL pointers
        assert f(None, 0, None) == (0 if have else no_device), name

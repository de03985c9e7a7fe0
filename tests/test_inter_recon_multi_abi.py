"""CPU: the declaration of kvz_hip_inter_recon_frames, motion compensation of several pictures over one shared pool of reference
pictures: declared, documented, exported with the kvz_ prefix and bound; kvz_hip_recon_picture in C99 and ctypes and in the header's
comments; the pool size and the ABI version; the older multi-picture sections point at the entry; the numpy convenience; without a
device the entry refuses before it looks at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRY = "kvz_hip_inter_recon_frames"
FIELDS = ("pred_y", "pred_u", "pred_v", "stride_y", "stride_c", "width", "height", "cus", "refs", "params")
OFFSETS = [0, 8, 16, 24, 28, 32, 36, 40, 48, 64]
SIZE = 104


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entry():
    L = _lib()
    from kvazaar_amd import _lib as B
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    assert ENTRY in A.declared_symbols() and hasattr(L, ENTRY) and hasattr(B.load(), ENTRY)
    assert re.search(r"\bT %s\b" % ENTRY, exported)
    res, args = B.SIGNATURES[ENTRY]
    params = [" ".join(p.split()) for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % ENTRY, src).group(1).split(",")]
    assert params == ["const kvz_hip_recon_picture *pictures", "int n_pictures", "const kvz_hip_ref_picture *pool", "int n_pool", "kvz_hip_stream s"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(B.ReconPicture), ctypes.c_int, ctypes.POINTER(B.RefPicture), ctypes.c_int, ctypes.c_void_p]


def test_struct_in_c99_and_ctypes_and_in_the_header_comments(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d %d", sizeof(kvz_hip_recon_picture), KVZ_HIP_RECON_POOL_PICTURES, KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_MAX_REF_PICTURES,',
             '         KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_recon_picture, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [SIZE, 48, 16, 16, 4] + OFFSETS
    assert B.RECON_POOL_PICTURES == 48
    assert ctypes.sizeof(B.ReconPicture) == SIZE and [getattr(B.ReconPicture, f).offset for f in FIELDS] == OFFSETS
    assert [f for f, _ in B.ReconPicture._fields_] == list(FIELDS)
    assert ctypes.sizeof(B.InterReconParams) == 40 and ctypes.sizeof(B.RefPicture) == 40
    # no implicit padding: the fields fill the record
    sizes = [getattr(B.ReconPicture, f).size for f in FIELDS]
    assert [o + s for o, s in zip(OFFSETS, sizes)] == OFFSETS[1:] + [SIZE]
    # the header states what the compiler says
    text = open(A.HEADER).read()
    decl = text[text.index("One picture of kvz_hip_inter_recon_frames"):text.index("} kvz_hip_recon_picture;")]
    decl = decl[decl.index("typedef struct {"):]
    stated = {}
    for line in decl.splitlines():
        m = re.match(r"\s*(?:const )?[\w ]+?[ *]([\w, *\[\]]+);\s*/\*\s*([\d, ]+?)\s*(?::|\*/)", line)
        if m:
            names = [re.sub(r"\[\d+\]", "", n).strip(" *") for n in m.group(1).split(",")]
            offs = [int(v) for v in m.group(2).split(",")]
            assert len(offs) == len(names), line
            stated.update(zip(names, offs))
    assert stated == dict(zip(FIELDS, OFFSETS))
    assert "} kvz_hip_recon_picture;                    /* 104 bytes, no implicit padding */" in text
    assert "#define KVZ_HIP_RECON_POOL_PICTURES 48" in text


def test_header_documents_the_entry():
    text = open(A.HEADER).read()
    doc = text[text.index("} kvz_hip_recon_picture;"):text.index("KVZ_HIP_API int " + ENTRY)]
    for what in ("THE RULE", "byte for byte", "kvz_hip_inter_recon_frame leaves", "refs[k] = pool[pictures[i].refs[k]]", "params.n_refs",
                 "left untouched", "picture-wide coordinates", "4:0:0 beside 4:2:0", "in a different order",
                 # the pool rules
                 "pool is HOST memory, copied at the call", "1..KVZ_HIP_RECON_POOL_PICTURES", "ignored entirely", "its fields are not looked at",
                 "must have the record's width and height", "without chroma planes", "k >= n_refs is not read",
                 # independence and the refusal list
                 "pred_y bases coincide", "named by any record", "no access leaves a record's", "n_pictures == 0 is a no-op", "pictures and pool may then be NULL",
                 "KVZ_HIP_ERR_INVALID", "outside 0..KVZ_HIP_MAX_CHAIN_PICTURES", "a NULL table", "record the single entry would refuse",
                 "refs[k] >= n_pool for a k < n_refs", "of another size or with missing planes", "the aliasing cases above",
                 "Every record is checked before anything is launched", "nothing is written for any picture", "picture 2", "KVZ_HIP_ERR_NO_DEVICE",
                 # execution
                 "one launch covers all pictures", "no host synchronisation, no allocation, no workspace", "3336 bytes, below 4 KB", "scalar loads",
                 "Usable between kvz_hip_graph_begin / _end", "depends only on the sizes", "CONTENTS of the CU arrays and of every plane changed",
                 "The ABI version stays 4"):
        assert what in doc, what
    # the three older multi-picture sections point at the entry and no longer say that it is not built
    for older in ("KVZ_HIP_API int kvz_hip_inter_residual_frames(", "KVZ_HIP_API int kvz_hip_inter_residual_frames_ts(", "KVZ_HIP_API int kvz_hip_cu_qp_frames("):
        before = text[:text.index(older)]
        tail = before[before.rindex("LEFT OUT ON PURPOSE"):]
        assert ENTRY in tail and "not built" not in tail, older
    single = text[text.index("kvz_inter_recon_cu (inter.c:492-540) for every inter CU"):text.index("KVZ_HIP_API int kvz_hip_inter_recon_frame(")]
    assert ENTRY in single


def test_numpy_convenience_exists():
    from kvazaar_amd import api
    assert list(inspect.signature(api.inter_recon_frames).parameters) == ["pictures", "pool"]


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_argument_checks_return_invalid_or_no_device():
    """with a device NULL tables, counts outside 0..16 and 1..48 and a record of NULL pointers are refused as invalid; without one the entry
    says so before it looks at anything"""
    import torch
    from kvazaar_amd import _lib as B
    f = getattr(B.load(), ENTRY)
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    records, pool = (B.ReconPicture * 17)(), (B.RefPicture * 49)()
    assert f(None, 1, pool, 1, None) == want and f(records, 1, None, 1, None) == want          # NULL tables
    assert f(records, 17, pool, 1, None) == want and f(records, -1, pool, 1, None) == want
    assert f(records, 1, pool, 0, None) == want and f(records, 1, pool, 49, None) == want
    assert f(records, 1, pool, 1, None) == want                                                # a record of NULL pointers
    assert f(None, 0, None, 0, None) == (0 if have else no_device)

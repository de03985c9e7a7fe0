"""CPU: the declarations of the two multi-picture entries with RDOQ -- kvz_hip_inter_residual_frames_rdoq and kvz_hip_intra_recon_frames_rdoq:
declared, documented, exported and bound; kvz_hip_chain_picture_rdoq in C, in ctypes and in the header's comments; the numpy conveniences;
the ABI version unchanged; the older paragraphs keep their sentences; the two new translation units keep RDOQ's doubles unfused; with a
device every argument check returns KVZ_HIP_ERR_INVALID, without one the entries say so before they look at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRIES = ("kvz_hip_inter_residual_frames_rdoq", "kvz_hip_intra_recon_frames_rdoq")
FIELDS = ("pic", "grid", "tables", "rdoq")
OFFSETS = [0, 160, 168, 184]


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
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name), name
        assert re.search(r"\bT %s\b" % name, exported), name
        res, args = B.SIGNATURES[name]
        params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1).split(",")]
        assert params == ["const kvz_hip_chain_picture_rdoq *pictures", "int n_pictures", "kvz_hip_stream s"], name
        assert res is ctypes.c_int and args == [ctypes.POINTER(B.ChainPictureRdoq), ctypes.c_int, ctypes.c_void_p], name


def test_struct_in_c_ctypes_and_the_headers_comments(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %d %d", sizeof(kvz_hip_chain_picture_rdoq), sizeof(kvz_hip_chain_picture), sizeof(kvz_hip_rdoq_source),',
             '         KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_chain_picture_rdoq, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [192, 160, 48, 16, 4] + OFFSETS
    assert ctypes.sizeof(B.ChainPictureRdoq) == 192 and [getattr(B.ChainPictureRdoq, f).offset for f in FIELDS] == OFFSETS
    assert [f for f, _ in B.ChainPictureRdoq._fields_] == list(FIELDS)
    # the header states what the compiler says
    text = open(A.HEADER).read()
    decl = text[text.index("One picture of kvz_hip_*_frames_rdoq"):text.index("} kvz_hip_chain_picture_rdoq;")]
    for f, off in zip(FIELDS, OFFSETS):
        assert re.search(r"[ *]%s;[^\n]*/\*\s*%d:" % (f, off), decl), (f, off)
    assert "} kvz_hip_chain_picture_rdoq;         /* 192 bytes */" in text


def test_header_documents_the_entries_and_the_older_paragraphs_stand():
    text = open(A.HEADER).read()
    at = text.index("} kvz_hip_chain_picture_rdoq;")
    assert at > text.index("KVZ_HIP_API int kvz_hip_intra_recon_frames_ts(")
    doc = text[at:text.index("KVZ_HIP_API int " + ENTRIES[0])]
    for what in ("THE RULE", "byte for byte", "kvz_hip_inter_residual_frame_rdoq", "kvz_hip_intra_recon_frame_rdoq", "which TUs take kvz_rdoq",
                 "an index >= n_sets used as n_sets - 1", "tr_depth from the record at the TU's own top-left SCU", "sign hiding", "the tile rule",
                 "4:0:0 beside 4:2:0", "tiled pictures beside untiled ones", "lcu_qp, cbf_out and costs", "ctx_sets, states,\n *   lcu_ctx and n_sets",
                 "ONE RESTRICTION", "homogeneous", "every record carries rdoq or none does", "rdoq->rdoq_skip, rdoq->tables.quant and rdoq->tables.err_scale",
                 "differs from record 0", "4 KB", "No rdoq at all", "kvz_hip_inter_residual_frames_ts", "ts == NULL", "names itself in kvz_hip_last_error",
                 "rec_y, cus or coeff_y base pointers coincide", "n_pictures == 0 is a no-op", "n_sets == 0", "not 16-byte aligned",
                 "KVZ_HIP_CHAIN_TILE_BOUNDS", "homogeneity, the record's own checks, its grid", "KVZ_HIP_ERR_INVALID", "writes nothing for any picture",
                 "names the record's index", "at which it overflowed", "no host synchronisation, no allocation, no workspace", "kvz_hip_graph_begin",
                 "CONTENTS", "w_t + 2 (h_t - 1)", "a wave per LCU", "a wave per TU", "one launch per TU width", "with rdoq_skip the 4x4 launch",
                 "OUT OF SCOPE", "transform skip together with RDOQ", "quantize_residual", "lossless", "bit depths above 8", "more than one lane",
                 "The ABI version stays 4"):
        assert what in doc, what
    # the older paragraphs keep their sentences word for word and gained a pointer to the new entries
    for old in ("OUT OF SCOPE: transform skip together with RDOQ (these entries take no kvz_hip_trskip), the multi-picture _frames / _frames_ts\n"
                " *   entries, the drop-in's quantize_residual, lossless, bit depths above 8, a recursion on more than one lane.",
                "(RDOQ exists as the batch entry kvz_hip_rdoq_batch,\n *   above; inside these stages it is still to come.)",
                "LEFT OUT ON PURPOSE: a call that mixes pictures with and without tables, or with and without ts",
                "this stage does not call it.", "these two stages still quantise with the rdoq-off path.", "these stages do not call it."):
        assert old in text, old
    assert text.count("_frames_rdoq entries") >= 2 and text.count("_rdoq entries further below") >= 2
    assert re.search(r"#define KVZ_HIP_ABI_VERSION 4\b", text)


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    for f, entry in ((api.inter_residual_frames_rdoq, ENTRIES[0]), (api.intra_recon_frames_rdoq, ENTRIES[1])):
        assert list(inspect.signature(f).parameters) == ["pictures"] and entry in f.__doc__
    p = inspect.signature(api._ChainPictureRdoq.__init__).parameters
    assert "rdoq" in p and "shared" in p
    # the staged kvz_hip_rdoq_source records live with the pictures, over the call
    assert "self.rq = _lib.RdoqSource(" in inspect.getsource(api._ChainPictureRdoq)
    # next to the _ts conveniences, not threaded through them
    assert "rdoq" not in inspect.getsource(api._chain_frames_ts) and "rdoq" not in inspect.getsource(api._ChainPictureTs)


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_argument_checks_return_invalid_or_no_device():
    """with a device NULL records, a count outside 0..16 and records that can only be refused are invalid; without one the entries say so
    before they look at anything"""
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    records = (B.ChainPictureRdoq * 17)()
    # never launched: a source whose ctx_sets is NULL, on a record of NULL pointers
    rq = B.RdoqSource(None, 0x5008, None, B.RdoqTables(0x7010, 0x8008), 6, 0)
    with_rdoq = (B.ChainPictureRdoq * 2)()
    with_rdoq[0].rdoq = ctypes.pointer(rq)
    for name in ENTRIES:
        f = getattr(L, name)
        assert f(None, 1, None) == want, name
        assert f(records, 17, None) == want and f(records, -1, None) == want, name
        # a record of NULL pointers, no rdoq: the _frames_ts entry answers (or, without any option, the _frames entry that it calls)
        assert f(records, 1, None) == want, name
        if have:
            assert name.replace("_rdoq", "").encode() in L.kvz_hip_last_error() and name.encode() not in L.kvz_hip_last_error()
        assert f(with_rdoq, 2, None) == want, name                        # with rdoq this entry answers, and names the record
        if have:
            assert name.encode() in L.kvz_hip_last_error() and b"picture 0 (" in L.kvz_hip_last_error()
        assert f(None, 0, None) == (0 if have else no_device), name


def test_the_new_kernels_doubles_stay_unfused_and_the_record_fits_the_arguments():
    csrc = os.path.join(A.ROOT, "kvazaar_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^\$\(OBJ\)/inter_residual_multi_rdoq\.o \$\(OBJ\)/intra_recon_multi_rdoq\.o: FLAGS \+= -ffp-contract=off$", make, flags=re.M)
    for unit in ("inter_residual_multi_rdoq.hip", "intra_recon_multi_rdoq.hip", "inter_residual_rdoq_core.h"):
        text = open(os.path.join(csrc, unit)).read()
        assert "#pragma clang fp contract(off)" in text and "asm" not in text and "-ffast-math" not in text, unit
        assert "hipMalloc" not in text and "hipStreamSynchronize" not in text and "hipDeviceSynchronize" not in text, unit
    core = open(os.path.join(csrc, "intra_recon_core.h")).read()
    assert "sizeof(intra_pic_rdoq) == 208" in core and "sizeof(intra_batch_rdoq<true>) + 8 <= 4096" in core
    for unit in ("inter_residual_multi_rdoq.hip", "intra_recon_multi_rdoq.hip"):
        text = open(os.path.join(csrc, unit)).read()
        # the checks are the walk's, which tests/test_chain_multi_rdoq_host_checks.py runs: the unit calls it and spells none itself
        assert "chain_records_why(pictures, n_pictures, " in text and "return refuse_picture(__func__, at, why);" in text, unit
        assert "chain_record_rdoq_why(" not in text and "chain_record_rdoq_shared(" not in text and "tile_pool_add(" not in text, unit

"""CPU: the declarations of RDOQ in the residual stages -- kvz_hip_inter_residual_frame_rdoq and kvz_hip_intra_recon_frame_rdoq declared,
documented, exported and bound; kvz_hip_rdoq_source in C99, in ctypes and in numpy; the ABI version unchanged; with a device every error
path returns KVZ_HIP_ERR_INVALID, without one the entries say so before they look at anything; the Python wrappers refuse rdoq together
with trskip; the translation units that hold RDOQ doubles keep them unfused."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_abi as A

INTER, INTRA = "kvz_hip_inter_residual_frame_rdoq", "kvz_hip_intra_recon_frame_rdoq"
FIELDS = ("ctx_sets", "states", "lcu_ctx", "tables", "n_sets", "rdoq_skip")
OFFSETS = [0, 8, 16, 24, 40, 44]


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def _params(text, entry):
    return [a.strip() for a in re.search(r"%s\((.*?)\);" % entry, text, flags=re.S).group(1).replace("\n", " ").split(",")]


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    for name in (INTER, INTRA):
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name), name
        assert re.search(r"\bT %s\b" % name, exported), name
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    sl, rq = ctypes.POINTER(B.ScalingTables), ctypes.POINTER(B.RdoqSource)
    assert B.SIGNATURES[INTER] == (I, [P, P, U, P, P, U, P, P, P, P, P, P, P, sl, rq, P, P])
    assert B.SIGNATURES[INTRA] == (I, [P, P, U, P, P, U, P, P, P, P, P, P, P, P, P, sl, rq, P, P])
    # the _sl entries with the record placed before params
    text = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    for entry, base in ((INTER, "kvz_hip_inter_residual_frame_sl"), (INTRA, "kvz_hip_intra_recon_frame_sl")):
        want = _params(text, base)
        want.insert(len(want) - 2, "const kvz_hip_rdoq_source *rdoq")
        assert _params(text, entry) == want, entry


def test_record_in_c99_ctypes_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %d", sizeof(kvz_hip_rdoq_source), KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_rdoq_source, %s));' % f for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [48, 4] + OFFSETS
    assert ctypes.sizeof(B.RdoqSource) == 48 and [getattr(B.RdoqSource, f).offset for f in FIELDS] == OFFSETS
    # the record as a numpy dtype with the alignment a C compiler gives it
    dt = np.dtype({"names": list(FIELDS), "formats": ["<u8", "<u8", "<u8", [("quant", "<u8"), ("err_scale", "<u8")], "<u4", "<i4"]}, align=True)
    assert dt.itemsize == 48 and [dt.fields[f][1] for f in FIELDS] == OFFSETS
    # the header states the same numbers
    text = open(A.HEADER).read()
    body = text[text.index("const kvz_hip_coeff_ctx  *ctx_sets;"):text.index("} kvz_hip_rdoq_source;")]
    assert [int(v) for v in re.findall(r"/\*\s*(\d+):", body)] == OFFSETS and "} kvz_hip_rdoq_source;          /* 48 bytes" in text


def test_header_documents_the_entries_and_what_stays_out():
    text = open(A.HEADER).read()
    at = text.index("RDOQ inside the two single-picture residual stages of the picture chain")
    assert at > text.index("Rate-distortion optimised quantisation (RDOQ) of a list of TUs")
    doc = text[at:text.index("Several independent pictures through the residual stages at once", at)]
    for phrase in ("quant-generic.c:214-221", "width > 4 || !rdoq_skip", "rdoq == NULL", "byte for byte", "kvz_hip_last_error", "states[].qp is",
                   "NOT read", "exactly the value the _sl entry quantises that TU with", "An index >= n_sets is used as n_sets - 1", "kvz_hip_coeff_pricing",
                   "always", "type 0 for Y and 2 for U and V", "kvz_get_scan_order", "block_type", "tr_depth - depth + (part_size == SIZE_NxN ? 1 : 0)",
                   "transform.c:437", "quant-generic.c:218-219", "clamped into 0..3", "qt_cbf_model_chroma[4]", "quant-generic.c:227-270", "has_coeffs",
                   "the prediction stands", "coeff_abs_*", "KVZ_HIP_ERR_INVALID", "n_sets == 0", "not 2-byte aligned", "not 8-byte aligned",
                   "not 16-byte aligned", "memory-safe", "finite lambda > 0", "no allocation", "no workspace", "no host synchronisation", "four launches",
                   "a wave per TU", "a wave per LCU", "kvz_hip_graph_begin", "CONTENTS", "ABI version stays 4", "OUT OF SCOPE", "kvz_hip_trskip",
                   "_frames / _frames_ts", "quantize_residual", "lossless", "bit depths above 8", "more than one lane"):
        assert phrase in doc, phrase
    # the older paragraphs keep their sentences and gained a pointer to the new entries
    for old in ("this stage does not call it.", "these two stages still quantise with the rdoq-off path.", "these stages do not call it."):
        assert old in text
    assert text.count("_rdoq entries further below") >= 2 and "kvz_hip_inter_residual_frame_rdoq\n *   (further below)" in text
    assert re.search(r"#define KVZ_HIP_ABI_VERSION 4\b", text)


def test_every_error_path_returns_invalid_or_no_device():
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    prm = np.zeros(6, np.int32)
    prm[0], prm[4] = 27, 1
    src = B.RefPicture(0x100000, 0x200000, 0x300000, 64, 32, 64, 64)

    def source(**kw):
        f = dict(ctx_sets=0x4002, states=0x5008, lcu_ctx=0x6002, quant=0x7010, err_scale=0x8008, n_sets=6, rdoq_skip=0)
        f.update(kw)
        return B.RdoqSource(f["ctx_sets"], f["states"], f["lcu_ctx"], B.RdoqTables(f["quant"], f["err_scale"]), f["n_sets"], f["rdoq_skip"])

    def call(entry, rq, **kw):
        # never launched: one argument is broken
        a = dict(src=ctypes.addressof(src), y=0x400000, sy=64, u=0x500000, v=0x600000, sc=32, cus=0x700000, modes=0x800000, cy=0x900000, cu=0xa00000,
                 cv=0xb00000, cbf=0xc00000, costs=0xd00000, lcu_qp=None, grid=None, tables=None, prm=prm.ctypes.data)
        a.update(kw)
        rq = ctypes.byref(rq) if rq is not None else None
        if entry == INTER:
            return L.kvz_hip_inter_residual_frame_rdoq(a["src"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["cy"], a["cu"], a["cv"], a["cbf"],
                                                       a["costs"], a["lcu_qp"], a["tables"], rq, a["prm"], None)
        return L.kvz_hip_intra_recon_frame_rdoq(a["src"], a["y"], a["sy"], a["u"], a["v"], a["sc"], a["cus"], a["modes"], a["cy"], a["cu"], a["cv"],
                                                a["cbf"], a["costs"], a["lcu_qp"], a["grid"], a["tables"], rq, a["prm"], None)

    broken = [dict(ctx_sets=None), dict(states=None), dict(quant=None), dict(err_scale=None), dict(n_sets=0), dict(ctx_sets=0x4001), dict(lcu_ctx=0x6001),
              dict(states=0x5004), dict(err_scale=0x8004), dict(quant=0x7008)]
    for entry in (INTER, INTRA):
        for kw in broken:
            assert call(entry, source(**kw)) == want, (entry, kw)
            if have:
                assert entry.encode() in L.kvz_hip_last_error()
        # a good record and a broken picture argument; rdoq == NULL and a broken picture argument (the _sl entry answers)
        for rq in (source(), None):
            for kw in (dict(src=None), dict(prm=None), dict(cus=None), dict(cy=0x900002), dict(sy=60)):
                assert call(entry, rq, **kw) == want, (entry, kw)
        if have:
            assert (entry.replace("_rdoq", "_sl")).encode() in L.kvz_hip_last_error()


def test_python_wrappers_refuse_rdoq_with_trskip_before_anything_else():
    from kvazaar_amd import api
    for f, args in ((api.inter_residual_frame, (None, None, None, 27)), (api.intra_recon_frame, (None, None, np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8), 27))):
        with pytest.raises(ValueError):
            f(*args, trskip=5, rdoq={})
    import inspect
    for f in (api.inter_residual_frame, api.intra_recon_frame):
        assert "rdoq" in inspect.signature(f).parameters and "kvz_hip_%s_rdoq" % ("inter_residual_frame" if f is api.inter_residual_frame else "intra_recon_frame") in f.__doc__


def test_the_stage_kernels_doubles_stay_unfused_and_stores_are_plain():
    csrc = os.path.join(A.ROOT, "kvazaar_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^\$\(OBJ\)/inter_residual_rdoq\.o \$\(OBJ\)/intra_recon_rdoq\.o: FLAGS \+= -ffp-contract=off$", make, flags=re.M)
    for unit in ("rdoq_stage.h", "inter_residual_rdoq.hip", "intra_recon_rdoq.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "#pragma clang fp contract(off)" in text and "asm" not in text and "-ffast-math" not in text, unit
    stage = open(os.path.join(csrc, "rdoq_stage.h")).read()
    for name in ("rdoq_prepare(", "rdoq_recursion(", "rdoq_finish(", "rdoq_sign_hide_group(", "rdoq_rd_factor(", "rdoq_make_tu(", "rdoq_state_byte("):
        assert name in stage, name
    # the helpers moved: rdoq.hip includes them and no longer defines them
    unit = open(os.path.join(csrc, "rdoq.hip")).read()
    assert '#include "rdoq_stage.h"' in unit and "rdoq_tu rdoq_make_tu(" not in unit
    # the cores without RDOQ never see the cost arithmetic
    for core in ("intra_recon_core.h", "inter_residual_core.h", "frame_sources.h"):
        assert '#include "rdoq' not in open(os.path.join(csrc, core)).read(), core

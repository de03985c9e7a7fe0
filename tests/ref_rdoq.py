"""The compiled reference's own kvz_rdoq (rdo.c:548-881), reached through tests/c_host/ref_rdoq.c: our glue, compiled here with gcc
against the reference's headers and oracle/_ref/libkvzref.so into a temporary directory.  The state kvz_rdoq runs on is fabricated
(see the C file): a zeroed encoder_control_t / encoder_state_t with the scaling lists processed by the reference itself.
available() is False where the reference's sources or the compiled library are absent; a machine with a GPU has neither, and no GPU test
uses this route.  TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ref_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "c_host", "ref_rdoq.c")
REF_SRC = os.path.join(os.environ.get("KVZ_REFERENCE", "/root/reference"), "src")      # oracle/Makefile: REF
CTX_BYTES = 184
SL_TABLE_LEN = 48960
CANARY = 0x5a5a
_LIB = None


def available():
    return ref_lib.available() and os.path.exists(os.path.join(REF_SRC, "rdo.h")) and shutil.which("gcc") is not None


def lib():
    global _LIB
    if _LIB is None:
        ref_lib.lib()                                           # loaded RTLD_GLOBAL and initialised (strategies selected)
        d = tempfile.mkdtemp(prefix="ref_rdoq_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libref_rdoq.so")
        ref_dir = os.path.dirname(ref_lib.REF_SO)
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-w", "-I" + REF_SRC, "-I" + os.path.join(REF_SRC, "extras"),
                               "-DKVZ_DLL_EXPORTS", SOURCE, "-o", so, "-L" + ref_dir, "-lkvzref", "-Wl,-rpath," + ref_dir])
        L = C.CDLL(so)
        L.rdoq_ref_ctx_bytes.restype = C.c_int
        L.rdoq_ref_ctx_offset.restype = C.c_int
        L.rdoq_ref_ctx_offset.argtypes = [C.c_int]
        L.rdoq_ref_init_contexts.restype = None
        L.rdoq_ref_init_contexts.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.rdoq_ref_run.restype = None
        L.rdoq_ref_run.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5
        L.rdoq_ref_quant_table.restype = C.POINTER(C.c_int32)
        L.rdoq_ref_quant_table.argtypes = [C.c_int] * 4
        L.rdoq_ref_err_table.restype = C.POINTER(C.c_double)
        L.rdoq_ref_err_table.argtypes = [C.c_int] * 4
        L.rdoq_ref_entropy_bits.restype = C.c_uint32
        L.rdoq_ref_entropy_bits.argtypes = [C.c_int]
        assert L.rdoq_ref_ctx_bytes() == CTX_BYTES
        _LIB = L
    return _LIB


def ctx_offsets():
    """(cu_qt_root_cbf_model, qt_cbf_model_luma, qt_cbf_model_chroma, cu_sig_coeff_group_model) as offsets into cabac_data_t.ctx"""
    L = lib()
    return tuple(L.rdoq_ref_ctx_offset(k) for k in range(4))


def init_contexts(qp, slice_type):
    """kvz_init_contexts for slice type 0 B / 1 P / 2 I: the 184 context bytes"""
    out = np.zeros(CTX_BYTES, dtype=np.uint8)
    lib().rdoq_ref_init_contexts(int(qp), int(slice_type), out.ctypes.data)
    return out


def tables(default_lists):
    """{(size_id, list, rem): (quant int32 [N * N], error_scale float64 [N * N])} of the lists the reference holds"""
    L = lib()
    out = {}
    for size_id in range(4):
        n = 16 << (2 * size_id)
        for list_id in range(6):
            if size_id == 3 and list_id not in (0, 1, 3):
                continue
            for rem in range(6):
                q = np.ctypeslib.as_array(L.rdoq_ref_quant_table(int(default_lists), size_id, list_id, rem), shape=(n,)).copy()
                e = np.ctypeslib.as_array(L.rdoq_ref_err_table(int(default_lists), size_id, list_id, rem), shape=(n,)).copy()
                out[(size_id, list_id, rem)] = (q, e)
    return out


def packed_tables(default_lists):
    """(quant int32 [SL_TABLE_LEN], err_scale float64 [SL_TABLE_LEN]) in the layout of kvz_hip_rdoq_tables, packed here in numpy"""
    quant, err = np.zeros(SL_TABLE_LEN, np.int32), np.zeros(SL_TABLE_LEN, np.float64)
    for (size_id, list_id, rem), (q, e) in tables(default_lists).items():
        at = 36 * (0, 16, 80, 336)[size_id] + (6 * list_id + rem) * q.size
        quant[at:at + q.size], err[at:at + q.size] = q, e
    return quant, err


def entropy_bits():
    L = lib()
    return [int(L.rdoq_ref_entropy_bits(i)) for i in range(128)]


def rdoq(coef, width, type_, scan_mode, block_type, tr_depth, qp, lam, ctx, signhide=1, default_lists=0):
    """kvz_rdoq on one TU -> dest_coeff int16 [width * width].  dest starts out filled with CANARY: what comes back shows that every
    value was written."""
    c = np.ascontiguousarray(coef, dtype=np.int16).ravel()
    assert c.size == width * width
    ctx = np.ascontiguousarray(ctx, dtype=np.uint8)
    assert ctx.size == CTX_BYTES
    dest = np.full(c.size, CANARY, dtype=np.int16)
    lib().rdoq_ref_run(ctx.ctypes.data, float(lam), int(qp), int(signhide), int(default_lists), c.ctypes.data, dest.ctypes.data, width, type_,
                       scan_mode, block_type, tr_depth)
    return dest

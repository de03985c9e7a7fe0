"""The compiled reference's own kvz_quantize_residual with cfg.rdoq_enable = 1, reached through tests/c_host/ref_quant_rdoq.c: our glue,
compiled here with gcc against the reference's headers and oracle/_ref/libkvzref.so into a temporary directory.  The reference decides
itself between kvz_rdoq and kvz_quant and derives tr_depth from the cu_info_t it is handed.  The state is fabricated (see the C file).
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
import ref_rdoq

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "c_host", "ref_quant_rdoq.c")
CTX_BYTES = ref_rdoq.CTX_BYTES
_LIB = None


def available():
    return ref_rdoq.available()


def lib():
    global _LIB
    if _LIB is None:
        ref_lib.lib()                                           # loaded RTLD_GLOBAL and initialised (strategies selected)
        d = tempfile.mkdtemp(prefix="ref_quant_rdoq_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libref_quant_rdoq.so")
        ref_dir = os.path.dirname(ref_lib.REF_SO)
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-fPIC", "-shared", "-w", "-I" + ref_rdoq.REF_SRC, "-I" + os.path.join(ref_rdoq.REF_SRC, "extras"),
                               "-DKVZ_DLL_EXPORTS", SOURCE, "-o", so, "-L" + ref_dir, "-lkvzref", "-Wl,-rpath," + ref_dir])
        L = C.CDLL(so)
        L.quant_rdoq_ref_ctx_bytes.restype = C.c_int
        L.quant_rdoq_ref_run.restype = C.c_int
        L.quant_rdoq_ref_run.argtypes = [C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 7
        assert L.quant_rdoq_ref_ctx_bytes() == CTX_BYTES
        _LIB = L
    return _LIB


def quantize_residual(ref_in, pred_in, width, color, scan_order, cu, qp, lam, ctx, rdoq_enable=1, rdoq_skip=0, signhide=0, default_lists=0,
                      slice_is_intra=0):
    """kvz_quantize_residual on one TU.  ref_in, pred_in: uint8 [width, width]; cu = (type, depth, tr_depth, part_size) of the record the
    reference is handed as cur_cu; ctx: the 184 context bytes.  -> (rec uint8 [width, width], coeff int16 [width * width], has_coeffs)"""
    r = np.ascontiguousarray(ref_in, dtype=np.uint8).reshape(width * width)
    p = np.ascontiguousarray(pred_in, dtype=np.uint8).reshape(width * width)
    ctx = np.ascontiguousarray(ctx, dtype=np.uint8)
    assert ctx.size == CTX_BYTES
    cfg = np.array([rdoq_enable, rdoq_skip, signhide, default_lists, slice_is_intra], dtype=np.int32)
    cu = np.array(cu, dtype=np.int32)
    tu = np.array([width, color, scan_order], dtype=np.int32)
    rec = np.full(width * width, 0x5a, dtype=np.uint8)
    coeff = np.full(width * width, ref_rdoq.CANARY, dtype=np.int16)
    has = lib().quant_rdoq_ref_run(ctx.ctypes.data, float(lam), int(qp), cfg.ctypes.data, cu.ctypes.data, tu.ctypes.data, r.ctypes.data, p.ctypes.data,
                                   rec.ctypes.data, coeff.ctypes.data)
    return rec.reshape(width, width), coeff, int(has != 0)

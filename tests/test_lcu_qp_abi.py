"""CPU: the three per-LCU-QP entries are declared, exported and bound; their structs and the Python records have the documented
layout; the numpy conveniences exist; the ABI version is unchanged."""
import ctypes
import inspect
import os
import re

import numpy as np

import test_abi as A
from patterns import CU_INFO


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_three_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    for name in ("kvz_hip_inter_residual_frame_qp", "kvz_hip_intra_recon_frame_qp", "kvz_hip_cu_qp_frame"):
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
    # the old entries' arguments with lcu_qp before params
    for old in ("kvz_hip_inter_residual_frame", "kvz_hip_intra_recon_frame"):
        res, args = B.SIGNATURES[old + "_qp"]
        was = B.SIGNATURES[old][1]
        assert res is ctypes.c_int and args == was[:-2] + [ctypes.c_void_p] + was[-2:]
    res, args = B.SIGNATURES["kvz_hip_cu_qp_frame"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4


def test_struct_sizes_and_python_records():
    from kvazaar_amd import api
    assert api.CU_QP_PARAMS.itemsize == 8 and api.CU_QP_PARAMS.names == ("start_qp", "chain_lcus")
    assert [api.CU_QP_PARAMS.fields[n][1] for n in api.CU_QP_PARAMS.names] == [0, 4]
    assert CU_INFO.itemsize == 20 and CU_INFO.fields["qp"][1] == 6 and CU_INFO.fields["depth"][1] == 1
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\}\s*kvz_hip_cu_qp_params;", src)
    assert m and re.findall(r"int32_t\s+(\w+);", m.group(1)) == ["start_qp", "chain_lcus"]
    # the header's declarations carry lcu_qp as a const int8_t array and lcu_last_qp as an int8_t array
    for name in ("kvz_hip_inter_residual_frame_qp", "kvz_hip_intra_recon_frame_qp", "kvz_hip_cu_qp_frame"):
        decl = re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1)
        assert "const int8_t *lcu_qp" in decl
    assert "int8_t *lcu_last_qp" in re.search(r"KVZ_HIP_API int kvz_hip_cu_qp_frame\(([^;]*)\);", src).group(1)


def test_numpy_conveniences():
    from kvazaar_amd import api
    assert inspect.signature(api.inter_residual_frame).parameters["lcu_qp"].default is None
    assert inspect.signature(api.intra_recon_frame).parameters["lcu_qp"].default is None
    p = inspect.signature(api.cu_qp_frame).parameters
    assert list(p) == ["cus", "cbf", "lcu_qp", "start_qp", "chain_lcus"] and p["chain_lcus"].default == 0
    assert np.dtype(np.int8).itemsize == 1


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4

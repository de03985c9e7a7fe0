"""CPU: kvz_hip_intra_recon_frame is declared, exported and bound with its 15 arguments, the numpy convenience exists, and the ABI
version is unchanged."""
import ctypes
import inspect
import os

import test_abi as A


def test_header_declares_and_library_exports_intra_recon():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(A.LIB)
    assert "kvz_hip_intra_recon_frame" in A.declared_symbols() and hasattr(L, "kvz_hip_intra_recon_frame")
    from kvazaar_amd import _lib, api
    res, args = _lib.SIGNATURES["kvz_hip_intra_recon_frame"]
    assert res is ctypes.c_int and len(args) == 15
    # the inter stage's arguments with intra_modes after cus
    inter = _lib.SIGNATURES["kvz_hip_inter_residual_frame"][1]
    assert args[:7] == inter[:7] and args[8:] == inter[7:]
    assert hasattr(_lib.load(), "kvz_hip_intra_recon_frame")
    assert list(inspect.signature(api.intra_recon_frame).parameters)[:8] == ["src", "rec", "cus", "modes", "qp", "chroma", "signhide", "slice_is_intra"]


def test_abi_version_is_still_4():
    L = ctypes.CDLL(A.LIB)
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4

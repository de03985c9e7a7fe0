"""CPU: the declarations of the two transform-skip entries: declared, exported and bound with the signatures of the _sl entries plus
the two new arguments; kvz_hip_trskip in C, ctypes and numpy; the ABI version is unchanged; without a device the entries refuse."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_abi as A

ENTRIES = {"kvz_hip_inter_residual_frame_ts": "kvz_hip_inter_residual_frame_sl", "kvz_hip_intra_recon_frame_ts": "kvz_hip_intra_recon_frame_sl"}


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    for name, old in ENTRIES.items():
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
        res, args = B.SIGNATURES[name]
        was = B.SIGNATURES[old][1]
        assert res is ctypes.c_int and args == was[:-2] + [ctypes.POINTER(B.TrSkip), ctypes.c_void_p] + was[-2:]
        params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1).split(",")]
        old_params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % old, src).group(1).split(",")]
        assert params[-4:-2] == ["const kvz_hip_trskip *ts", "uint8_t *tr_skip_out"] and params[:-4] + params[-2:] == old_params, name


def test_struct_in_c_ctypes_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B, api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu %d\\n", sizeof(kvz_hip_trskip), offsetof(kvz_hip_trskip, bit_cost), offsetof(kvz_hip_trskip, reserved),'
             ' offsetof(kvz_hip_trskip, lcu_bit_cost), KVZ_HIP_ABI_VERSION);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [16, 0, 4, 8, 4]
    assert ctypes.sizeof(B.TrSkip) == 16 and [getattr(B.TrSkip, f).offset for f in ("bit_cost", "reserved", "lcu_bit_cost")] == [0, 4, 8]
    assert api.TRSKIP.itemsize == 16 and [api.TRSKIP.fields[f][1] for f in ("bit_cost", "reserved", "lcu_bit_cost")] == [0, 4, 8]
    assert np.zeros(1, api.TRSKIP).nbytes == 16


def test_numpy_conveniences_take_trskip():
    from kvazaar_amd import api
    for f in (api.inter_residual_frame, api.intra_recon_frame):
        p = inspect.signature(f).parameters
        assert p["trskip"].default is None and p["tr_skip"].default is None and p["scaling"].default is None


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_without_a_device_the_entries_return_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kvazaar_amd import _lib as B
    L = B.load()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", open(A.HEADER).read()).group(1))
    for name in ENTRIES:
        args = [0 if t is ctypes.c_uint32 else None for t in B.SIGNATURES[name][1]]
        assert getattr(L, name)(*args) == no_device, name

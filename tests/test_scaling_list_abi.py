"""CPU: kvz_hip_scaling_tables_pack (host only) and the declarations of the two scaling-list entries: declared, exported and bound with
the signatures of the entries they extend plus the tables; kvz_hip_scaling_tables and KVZ_HIP_SL_TABLE_LEN in C, ctypes and numpy;
the ABI version is unchanged; without a device the entries refuse."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import scaling_list_cases as SL
import test_abi as A

ENTRIES = {"kvz_hip_inter_residual_frame_sl": "kvz_hip_inter_residual_frame_qp", "kvz_hip_intra_recon_frame_sl": "kvz_hip_intra_recon_frame_tiles"}
INVALID = -2                                                          # KVZ_HIP_ERR_INVALID


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def _tables():
    return SL.process_lists(*SL.custom_lists())


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    assert int(re.search(r"KVZ_HIP_ERR_INVALID\s*=\s*(-?\d+)", src).group(1)) == INVALID
    assert "kvz_hip_scaling_tables_pack" in A.declared_symbols() and hasattr(L, "kvz_hip_scaling_tables_pack")
    for name, old in ENTRIES.items():
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
        res, args = B.SIGNATURES[name]
        was = B.SIGNATURES[old][1]
        assert res is ctypes.c_int and args == was[:-2] + [ctypes.POINTER(B.ScalingTables)] + was[-2:]
        params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1).split(",")]
        old_params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % old, src).group(1).split(",")]
        assert params[-3] == "const kvz_hip_scaling_tables *tables" and params[:-3] + params[-2:] == old_params, name


def test_struct_and_macro_in_c_ctypes_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B, api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%d %zu %zu %zu %d\\n", KVZ_HIP_SL_TABLE_LEN, sizeof(kvz_hip_scaling_tables), offsetof(kvz_hip_scaling_tables, quant),'
             ' offsetof(kvz_hip_scaling_tables, dequant), KVZ_HIP_ABI_VERSION);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [48960, 16, 0, 8, 4]
    assert ctypes.sizeof(B.ScalingTables) == 16 and [getattr(B.ScalingTables, f).offset for f in ("quant", "dequant")] == [0, 8]
    assert B.SL_TABLE_LEN == api.SL_TABLE_LEN == SL.TABLE_LEN == 48960 == 36 * (16 + 64 + 256 + 1024)
    assert np.zeros(api.SL_TABLE_LEN, np.int32).nbytes == 195840


def test_offsets_are_the_documented_layout():
    from kvazaar_amd import api
    seen = []
    for s in range(4):
        for l in range(6):
            for r in range(6):
                at = api.sl_table_offset(s, l, r)
                assert at == SL.table_offset(s, l, r) == 36 * (0, 16, 80, 336)[s] + (6 * l + r) * (4 << s) ** 2 and at % 4 == 0
                seen.append((at, at + (4 << s) ** 2))
    assert seen[0][0] == 0 and seen[-1][1] == api.SL_TABLE_LEN and all(a[1] == b[0] for a, b in zip(seen, seen[1:]))


def test_numpy_conveniences_take_scaling():
    from kvazaar_amd import api
    for f in (api.inter_residual_frame, api.intra_recon_frame):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "scaling" and p["scaling"].default is None


def test_pack_lays_the_tables_out_and_handles_the_32x32_aliases():
    from kvazaar_amd import api
    t = _tables()
    q, d = api.pack_scaling_tables({k: v[0] for k, v in t.items()}, {k: v[1] for k, v in t.items()})
    wq, wd = SL.dense(t)
    assert q.dtype == np.int32 and q.shape == (api.SL_TABLE_LEN,)
    np.testing.assert_array_equal(q, wq)
    np.testing.assert_array_equal(d, wd)
    for r in range(6):
        for a in (q, d):
            at = [api.sl_table_offset(3, l, r) for l in range(6)]
            assert not a[at[2]:at[2] + 1024].any() and not a[at[4]:at[4] + 1024].any() and not a[at[5]:at[5] + 1024].any()
            np.testing.assert_array_equal(a[at[3]:at[3] + 1024], a[at[1]:at[1] + 1024])
            assert a[at[0]:at[0] + 1024].all() and a[at[1]:at[1] + 1024].all()
    # nested sequences work as well as dicts
    nested = [[[t[(s, l, r)][0] if (s, l, r) in t else None for r in range(6)] for l in range(6)] for s in range(4)]
    q2, _ = api.pack_scaling_tables(nested, {k: v[1] for k, v in t.items()})
    np.testing.assert_array_equal(q2, wq)


def _pointer_arrays(t, poison_unused=False, drop=None):
    keep, out = [], []
    for which in (0, 1):
        p = (ctypes.c_void_p * 6 * 6 * 4)()
        for s in range(4):
            for l in range(6):
                for r in range(6):
                    if (s, l, r) in t and (s, l, r, which) != drop:
                        a = np.ascontiguousarray(t[(s, l, r)][which])
                        keep.append(a)
                        p[s][l][r] = a.ctypes.data
                    elif (s, l, r) not in t and poison_unused:
                        p[s][l][r] = 0x10                              # not a mapped address: reading it would fault
        out.append(p)
    return out, keep


def test_pack_does_not_read_the_unset_32x32_pointers_and_refuses_a_null():
    L = _lib()
    t = _tables()
    f = L.kvz_hip_scaling_tables_pack
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] * 4
    wq, wd = SL.dense(t)
    q, d = np.full(SL.TABLE_LEN, -7, np.int32), np.full(SL.TABLE_LEN, -7, np.int32)
    (pq, pd), keep = _pointer_arrays(t, poison_unused=True)
    assert f(ctypes.addressof(pq), ctypes.addressof(pd), q.ctypes.data, d.ctypes.data) == 0
    np.testing.assert_array_equal(q, wq)
    np.testing.assert_array_equal(d, wd)
    for drop in ((0, 0, 0, 0), (1, 5, 3, 1), (2, 2, 5, 0), (3, 0, 0, 1), (3, 1, 2, 0), (3, 3, 4, 1)):
        (pq, pd), keep = _pointer_arrays(t, drop=drop)
        q[:] = -7
        d[:] = -7
        assert f(ctypes.addressof(pq), ctypes.addressof(pd), q.ctypes.data, d.ctypes.data) == INVALID, drop
        assert (q == -7).all() and (d == -7).all(), "nothing is written"
    (pq, pd), keep = _pointer_arrays(t)
    assert f(None, ctypes.addressof(pd), q.ctypes.data, d.ctypes.data) == INVALID
    assert f(ctypes.addressof(pq), ctypes.addressof(pd), None, d.ctypes.data) == INVALID
    L.kvz_hip_last_error.restype = ctypes.c_char_p
    assert b"kvz_hip_scaling_tables_pack" in L.kvz_hip_last_error()


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

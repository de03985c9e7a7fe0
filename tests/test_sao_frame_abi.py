"""CPU: kvz_hip_sao_stats_frame and kvz_hip_sao_frame are declared, exported and bound, the numpy record types of kvazaar_amd/api.py
match sizeof / offsetof of their structs in include/kvz_hip.h as a C compiler lays them out, and the ABI version is unchanged."""
import ctypes
import os
import subprocess

import test_abi as A

ENTRIES = {"kvz_hip_sao_stats_frame": 10, "kvz_hip_sao_frame": 16}


def test_header_declares_and_library_exports_the_sao_frame_entries():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(A.LIB)
    from kvazaar_amd import _lib, api
    for name, n_args in ENTRIES.items():
        assert name in A.declared_symbols() and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(_lib.load(), name)
    assert callable(api.sao_stats_frame) and callable(api.sao_frame)


def test_sao_frame_record_layouts_match_the_header(tmp_path):
    from kvazaar_amd import api
    import sao_frame_cases as SC
    pairs = [("kvz_hip_sao_lcu_stats", api.SAO_LCU_STATS), ("kvz_hip_sao_lcu_cand", api.SAO_LCU_CAND), ("kvz_hip_sao_info", api.SAO_INFO),
             ("kvz_hip_ref_picture", api.REF_PICTURE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {', '  printf("abi %d\\n", KVZ_HIP_ABI_VERSION);']
    for cname, dt in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field in dt.names:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ['  printf("edge_dims %zu %zu\\n", sizeof(((kvz_hip_sao_lcu_stats *)0)->edge[0]), sizeof(((kvz_hip_sao_lcu_stats *)0)->edge[0][0]));',
              '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    got = dict(line.split() for line in out if not line.startswith("edge_dims "))
    assert int(got["abi"]) == 4
    for cname, dt in pairs:
        assert int(got[cname]) == dt.itemsize, cname
        for field in dt.names:
            assert int(got["%s.%s" % (cname, field)]) == dt.fields[field][1], "%s.%s" % (cname, field)
    assert (api.SAO_LCU_STATS.itemsize, api.SAO_LCU_CAND.itemsize, api.SAO_INFO.itemsize) == (416, 120, 56)
    assert [line for line in out if line.startswith("edge_dims ")][0].split()[1:] == ["40", "20"]         # edge[4][2][5]
    assert SC.STATS == api.SAO_LCU_STATS and SC.CAND == api.SAO_LCU_CAND


def test_abi_version_is_still_4():
    L = ctypes.CDLL(A.LIB)
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4

"""CPU: kvz_hip_inter_residual_frame is declared, exported and bound, the numpy record types of kvazaar_amd/api.py match sizeof /
offsetof of its structs in include/kvz_hip.h as a C compiler lays them out, and the ABI version is unchanged."""
import ctypes
import os
import subprocess

import test_abi as A


def test_header_declares_and_library_exports_inter_residual():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(A.LIB)
    assert "kvz_hip_inter_residual_frame" in A.declared_symbols() and hasattr(L, "kvz_hip_inter_residual_frame")
    from kvazaar_amd import _lib
    assert len(_lib.SIGNATURES["kvz_hip_inter_residual_frame"][1]) == 14
    assert hasattr(_lib.load(), "kvz_hip_inter_residual_frame")


def test_inter_residual_record_layouts_match_the_header(tmp_path):
    from kvazaar_amd import api
    import inter_residual_cases as RC
    pairs = [("kvz_hip_inter_residual_params", api.INTER_RESIDUAL_PARAMS), ("kvz_hip_inter_residual_cost", api.INTER_RESIDUAL_COST),
             ("kvz_hip_ref_picture", api.REF_PICTURE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {', '  printf("abi %d\\n", KVZ_HIP_ABI_VERSION);',
             '  printf("quant %zu %zu %zu %zu\\n", offsetof(kvz_hip_quant_params, qp), offsetof(kvz_hip_quant_params, slice_is_intra),',
             '         offsetof(kvz_hip_quant_params, signhide), offsetof(kvz_hip_quant_params, scaling_list));']
    for cname, dt in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field in dt.names:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    got = dict(line.split() for line in out if not line.startswith("quant "))
    assert int(got["abi"]) == 4
    for cname, dt in pairs:
        assert int(got[cname]) == dt.itemsize, cname
        for field in dt.names:
            assert int(got["%s.%s" % (cname, field)]) == dt.fields[field][1], "%s.%s" % (cname, field)
    assert (api.INTER_RESIDUAL_PARAMS.itemsize, api.INTER_RESIDUAL_COST.itemsize) == (24, 24)
    # the params struct embeds the first four fields of kvz_hip_quant_params at their offsets
    q = [line for line in out if line.startswith("quant ")][0].split()[1:]
    assert [int(v) for v in q] == [api.INTER_RESIDUAL_PARAMS.fields[f][1] for f in ("qp", "slice_is_intra", "signhide", "scaling_list")]
    assert RC.COST == api.INTER_RESIDUAL_COST


def test_abi_version_is_still_4():
    L = ctypes.CDLL(A.LIB)
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4

"""CPU: the two motion-compensation entries are declared and exported, and the numpy record types of kvazaar_amd/api.py match
sizeof / offsetof of their structs in include/kvz_hip.h as a C compiler lays them out."""
import ctypes
import os
import subprocess

import test_abi as A


def test_header_declares_and_library_exports_inter_recon():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    syms = A.declared_symbols()
    L = ctypes.CDLL(A.LIB)
    for s in ("kvz_hip_inter_recon_batch", "kvz_hip_inter_recon_frame"):
        assert s in syms, s
        assert hasattr(L, s), s
    from kvazaar_amd import _lib
    assert len(_lib.SIGNATURES["kvz_hip_inter_recon_batch"][1]) == 11 and len(_lib.SIGNATURES["kvz_hip_inter_recon_frame"][1]) == 11


def test_inter_recon_record_layouts_match_the_header(tmp_path):
    from kvazaar_amd import api
    pairs = [("kvz_hip_ref_picture", api.REF_PICTURE), ("kvz_hip_inter_pu", api.INTER_PU), ("kvz_hip_inter_recon_params", api.INTER_RECON_PARAMS)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("max_refs %d\\n", KVZ_HIP_MAX_REF_PICTURES);', '  printf("abi %d\\n", KVZ_HIP_ABI_VERSION);']
    for cname, dt in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field in dt.names:
            if field != "pad":
                lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["max_refs"]) == 16 and int(got["abi"]) == 4
    for cname, dt in pairs:
        assert int(got[cname]) == dt.itemsize, cname
        for field in dt.names:
            if field != "pad":
                assert int(got["%s.%s" % (cname, field)]) == dt.fields[field][1], "%s.%s" % (cname, field)
    assert (api.REF_PICTURE.itemsize, api.INTER_PU.itemsize, api.INTER_RECON_PARAMS.itemsize) == (40, 28, 40)

"""CPU: the declarations of RDOQ on the device -- kvz_hip_rdoq_batch and kvz_hip_rdoq_tables_pack declared, documented, exported and bound;
kvz_hip_rdoq_tables, kvz_hip_rdoq_state, kvz_hip_rdoq_desc and kvz_hip_rdoq_params in C99, in ctypes / numpy and in the header's comments; the
ABI version unchanged; the pack function against the fixture's tables and its NULL errors; the argument checks of
kvazaar_amd/csrc/rdoq_host.h as a host program; with a device every error path returns KVZ_HIP_ERR_INVALID, without one the entry says so
before it looks at anything; the helper that cuts a state record from a context dump; the two switches that keep the kernels' doubles
unfused."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_abi as A

ENTRY, PACK = "kvz_hip_rdoq_batch", "kvz_hip_rdoq_tables_pack"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rdoq.npz")


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    for name in (ENTRY, PACK):
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name), name
        assert re.search(r"\bT %s\b" % name, exported), name
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert B.SIGNATURES[ENTRY] == (I, [P, P, P, ctypes.c_size_t, P, P, U, ctypes.POINTER(B.RdoqTables), ctypes.POINTER(B.RdoqParams), P])
    assert B.SIGNATURES[PACK] == (I, [P, P, P, P])
    text = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    params = [a.strip() for a in re.search(r"%s\((.*?)\);" % ENTRY, text, flags=re.S).group(1).replace("\n", " ").split(",")]
    assert params == ["const kvz_hip_coeff *coef", "kvz_hip_coeff *dest", "const kvz_hip_rdoq_desc *descs", "size_t n", "const kvz_hip_coeff_ctx *ctx_sets",
                      "const kvz_hip_rdoq_state *states", "uint32_t n_sets", "const kvz_hip_rdoq_tables *tables", "const kvz_hip_rdoq_params *params",
                      "kvz_hip_stream s"]


STATE_FIELDS = ("lambda", "qp", "root_cbf", "qt_cbf_luma", "qt_cbf_chroma", "reserved")
DESC_FIELDS = ("src_offset", "dst_offset", "width", "type", "scan_mode", "block_type", "tr_depth", "reserved", "ctx_index")


def test_structs_in_c99_ctypes_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B, api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu %d", sizeof(kvz_hip_rdoq_tables), sizeof(kvz_hip_rdoq_state), sizeof(kvz_hip_rdoq_desc), sizeof(kvz_hip_rdoq_params),',
             '         KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_rdoq_tables, %s));' % f for f in ("quant", "err_scale")]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_rdoq_state, %s));' % f for f in STATE_FIELDS]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_rdoq_desc, %s));' % f for f in DESC_FIELDS]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_rdoq_params, %s));' % f for f in ("signhide", "reserved")]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    state_at, desc_at = [0, 8, 9, 10, 14, 18], [0, 4, 8, 9, 10, 11, 12, 13, 14]
    assert got == [16, 24, 16, 16, 4] + [0, 8] + state_at + desc_at + [0, 4]
    assert ctypes.sizeof(B.RdoqTables) == 16 and [getattr(B.RdoqTables, f).offset for f in ("quant", "err_scale")] == [0, 8]
    assert ctypes.sizeof(B.RdoqParams) == 16 and [getattr(B.RdoqParams, f).offset for f in ("signhide", "reserved")] == [0, 4]
    assert api.RDOQ_STATE.itemsize == 24 and [api.RDOQ_STATE.fields[f][1] for f in STATE_FIELDS] == state_at
    assert api.RDOQ_DESC.itemsize == 16 and [api.RDOQ_DESC.fields[f][1] for f in DESC_FIELDS] == desc_at
    assert (api.CU_INTRA, api.CU_INTER) == (1, 2)


def test_header_documents_the_entry_and_what_stays_out():
    text = open(A.HEADER).read()
    at = text.index("Rate-distortion optimised quantisation (RDOQ) of a list of TUs")
    assert at > text.index("Lossless coding in the picture chain")
    doc = text[at:text.index("Several independent pictures through the residual stages at once", at)]
    for phrase in ("rdo.c:548-881", "rdo.c:233-278", "rdo.c:297-339", "rdo.c:350-395", "rdo.c:405-539", "quant-generic.c:214-221", "scalinglist.c:339-356",
                   "rdo.c:563-564", "rdo.c:629", "rdo.c:759-812", ":815-864", ":866-876", "cu.h:39-41", "cabac.h:61-62", "KVZ_HIP_SL_TABLE_LEN",
                   "kvz_hip_scaling_tables_pack", "always required", "64-bit product", "no fused multiply-add", "binary64", "must not overlap",
                   "left untouched", "KVZ_HIP_ERR_INVALID", "n == 0", "kvz_hip_graph_begin", "CONTENTS", "ABI version stays 4", "multiples of 4",
                   "z-order", "abs_sum >= 2", "order or the grouping", "OUT OF SCOPE", "_frames_ts", "quantize_residual", "bit depths above 8",
                   "(byte >> 1) & 63", "All N * N"):
        assert phrase in doc, phrase
    # the older sections keep their sentences and the pricing section's record is the one this entry reads
    assert "OUT OF SCOPE: RDOQ (its lambda, error_scale and" in text and "OUT OF SCOPE: RDOQ and its error_scale" in text
    assert re.search(r"#define KVZ_HIP_ABI_VERSION 4\b", text)


def test_pack_against_the_fixture_and_its_null_errors():
    from kvazaar_amd import api, _lib as B
    import rdoq_model as M
    z = np.load(FIXTURE)
    for sl in (0, 1):
        quant, err = {}, {}
        for size_id in range(4):
            n = 16 << (2 * size_id)
            for list_id in range(6):
                if size_id == 3 and list_id not in (0, 1, 3):
                    continue
                for rem in range(6):
                    at = M.table_offset(size_id, list_id, rem)
                    quant[(size_id, list_id, rem)] = z["quant"][sl][at:at + n]
                    err[(size_id, list_id, rem)] = z["err_scale"][sl][at:at + n]
        q, e = api.pack_rdoq_tables(quant, err)
        assert q.dtype == np.int32 and e.dtype == np.float64 and q.size == e.size == api.SL_TABLE_LEN
        assert (q == z["quant"][sl]).all() and (e.view(np.uint64) == z["err_scale"][sl].view(np.uint64)).all()
        for list_id in (2, 4, 5):                                   # the 32x32 tables nobody holds are zeros
            at = M.table_offset(3, list_id, 0)
            assert not q[at:at + 6 * 1024].any() and not e[at:at + 6 * 1024].any()
        # a list of size 3 that is read, missing: refused
        del quant[(3, 3, 2)]
        with pytest.raises(B.KvzHipError):
            api.pack_rdoq_tables(quant, err)
    L = B.load()
    ptrs = (ctypes.c_void_p * 144)()
    out = np.zeros(api.SL_TABLE_LEN, np.float64)
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", open(A.HEADER).read()).group(1))
    for args in ((None, ptrs, out.ctypes.data, out.ctypes.data), (ptrs, None, out.ctypes.data, out.ctypes.data), (ptrs, ptrs, None, out.ctypes.data),
                 (ptrs, ptrs, out.ctypes.data, None), (ptrs, ptrs, out.ctypes.data, out.ctypes.data)):
        assert L.kvz_hip_rdoq_tables_pack(*args) == invalid
    assert not out.any()


def test_state_record_from_a_dump():
    from kvazaar_amd import api
    dump = np.arange(184, dtype=np.uint8)
    rec = api.rdoq_state_from_dump(dump, 4.25, 37)
    assert rec["lambda"] == 4.25 and rec["qp"] == 37 and rec["root_cbf"] == 181
    assert rec["qt_cbf_luma"].tolist() == [16, 17, 18, 19] and rec["qt_cbf_chroma"].tolist() == [20, 21, 22, 23] and not rec["reserved"].any()
    for bad in (lambda: api.rdoq_state_from_dump(dump[:183], 1.0, 30), lambda: api.rdoq_state_from_dump(dump, 1.0, -1),
                lambda: api.rdoq_state_from_dump(dump, 1.0, 52)):
        with pytest.raises(ValueError):
            bad()
    # the record's layout is the model's reading of the reference's block, next to the one coeff_ctx_from_dump cuts
    import rdoq_model as M
    assert (M.QT_CBF_LUMA, M.QT_CBF_CHROMA, M.ROOT_CBF) == (16, 20, 181)
    assert api.coeff_ctx_from_dump(dump, 300)["ctx"][:4].tolist() == [32, 33, 34, 35]


def test_every_error_path_returns_invalid_or_no_device():
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    f = L.kvz_hip_rdoq_batch
    prm = B.RdoqParams(1)
    names = ("coef", "dest", "descs", "n", "ctx_sets", "states", "n_sets", "tables", "params")

    def call(quant=0x7000, err_scale=0x8000, **kw):
        tab = B.RdoqTables(quant, err_scale)
        a = [0x1000, 0x2000, 0x3000, 1, 0x4000, 0x5000, 1, ctypes.pointer(tab), ctypes.pointer(prm), None]   # never launched: one argument is broken
        for k, v in kw.items():
            a[names.index(k)] = v
        return f(*a)

    for broken in (dict(coef=None), dict(dest=None), dict(descs=None), dict(ctx_sets=None), dict(states=None), dict(tables=None), dict(params=None),
                   dict(quant=None), dict(err_scale=None), dict(n_sets=0), dict(n=1 << 31), dict(coef=0x1004), dict(dest=0x2004), dict(descs=0x3002),
                   dict(ctx_sets=0x4001), dict(states=0x5004), dict(quant=0x7008), dict(err_scale=0x8004)):
        assert call(**broken) == want, broken
        if have:
            assert ENTRY.encode() in L.kvz_hip_last_error()
    # nothing to do is not an error, whatever the pointers are
    assert f(None, None, None, 0, None, None, 0, None, None, None) == (0 if have else no_device)


PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "kvz_hip.h"
#include "rdoq_host.h"

int main()
{
  const kvz_hip_coeff *c = (const kvz_hip_coeff *)0x1000, *o = (const kvz_hip_coeff *)0x2008;
  const kvz_hip_rdoq_desc *d = (const kvz_hip_rdoq_desc *)0x3004;
  const kvz_hip_coeff_ctx *s = (const kvz_hip_coeff_ctx *)0x4002;
  const kvz_hip_rdoq_state *t = (const kvz_hip_rdoq_state *)0x5008;
  kvz_hip_rdoq_tables tab = { (const int32_t *)0x7010, (const double *)0x8008 }, no_quant = { nullptr, (const double *)0x8008 },
                      no_err = { (const int32_t *)0x7010, nullptr }, quant8 = { (const int32_t *)0x7008, (const double *)0x8008 },
                      err4 = { (const int32_t *)0x7010, (const double *)0x8004 };
  kvz_hip_rdoq_params p = { 1, { 0, 0, 0 } };
  struct { const char *name; const char *why; } r[] = {
    { "clean", rdoq_batch_why(c, o, d, 5, s, t, 1, &tab, &p) },
    { "largest n", rdoq_batch_why(c, o, d, 0x7fffffffu, s, t, 1, &tab, &p) },
    { "coef null", rdoq_batch_why(nullptr, o, d, 5, s, t, 1, &tab, &p) },
    { "dest null", rdoq_batch_why(c, nullptr, d, 5, s, t, 1, &tab, &p) },
    { "descs null", rdoq_batch_why(c, o, nullptr, 5, s, t, 1, &tab, &p) },
    { "sets null", rdoq_batch_why(c, o, d, 5, nullptr, t, 1, &tab, &p) },
    { "states null", rdoq_batch_why(c, o, d, 5, s, nullptr, 1, &tab, &p) },
    { "tables null", rdoq_batch_why(c, o, d, 5, s, t, 1, nullptr, &p) },
    { "params null", rdoq_batch_why(c, o, d, 5, s, t, 1, &tab, nullptr) },
    { "quant null", rdoq_batch_why(c, o, d, 5, s, t, 1, &no_quant, &p) },
    { "err null", rdoq_batch_why(c, o, d, 5, s, t, 1, &no_err, &p) },
    { "no sets", rdoq_batch_why(c, o, d, 5, s, t, 0, &tab, &p) },
    { "n too large", rdoq_batch_why(c, o, d, (size_t)1 << 31, s, t, 1, &tab, &p) },
    { "coef at 4", rdoq_batch_why((const kvz_hip_coeff *)0x1004, o, d, 5, s, t, 1, &tab, &p) },
    { "dest at 4", rdoq_batch_why(c, (const kvz_hip_coeff *)0x2004, d, 5, s, t, 1, &tab, &p) },
    { "descs at 2", rdoq_batch_why(c, o, (const kvz_hip_rdoq_desc *)0x3002, 5, s, t, 1, &tab, &p) },
    { "sets at 1", rdoq_batch_why(c, o, d, 5, (const kvz_hip_coeff_ctx *)0x4001, t, 1, &tab, &p) },
    { "states at 4", rdoq_batch_why(c, o, d, 5, s, (const kvz_hip_rdoq_state *)0x5004, 1, &tab, &p) },
    { "quant at 8", rdoq_batch_why(c, o, d, 5, s, t, 1, &quant8, &p) },
    { "err at 4", rdoq_batch_why(c, o, d, 5, s, t, 1, &err4, &p) },
    { "null before no sets", rdoq_batch_why(nullptr, o, d, 5, s, t, 0, &tab, &p) },
  };
  for (auto &e : r) printf("%s: %s\n", e.name, e.why ? e.why : "ok");
  return 0;
}
"""
NULL, TABLE, SETS, COUNT = "a pointer is null", "a table is null", "n_sets is 0", "n above 2^31 - 1"
ALIGN = "coef, dest or states not 8-byte, descs not 4-byte or ctx_sets not 2-byte aligned"
TALIGN = "quant not 16-byte or err_scale not 8-byte aligned"
EXPECTED = {"clean": "ok", "largest n": "ok", "coef null": NULL, "dest null": NULL, "descs null": NULL, "sets null": NULL, "states null": NULL,
            "tables null": NULL, "params null": NULL, "quant null": TABLE, "err null": TABLE, "no sets": SETS, "n too large": COUNT, "coef at 4": ALIGN,
            "dest at 4": ALIGN, "descs at 2": ALIGN, "sets at 1": ALIGN, "states at 4": ALIGN, "quant at 8": TALIGN, "err at 4": TALIGN,
            "null before no sets": NULL}


def test_argument_checks_as_a_host_program(tmp_path):
    """rdoq_host.h takes a plain C++17 compiler with kvz_hip.h alone: the checks compare pointers and follow none but the two HOST structs"""
    src, exe = tmp_path / "rdoq_checks.cpp", tmp_path / "rdoq_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(A.ROOT, "include"), "-I", os.path.join(A.ROOT, "kvazaar_amd", "csrc"), str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    assert got == EXPECTED


def test_the_kernels_doubles_stay_unfused_and_the_tables_are_shared():
    """the reference's object code fuses nothing: contraction is off in the core header and on the translation unit's compile line"""
    csrc = os.path.join(A.ROOT, "kvazaar_amd", "csrc")
    core, unit, make, tables, cabac = (open(os.path.join(csrc, n)).read() for n in ("rdoq_core.h", "rdoq.hip", "Makefile", "cabac_tables.h", "coeff_cabac_core.h"))
    assert "#pragma clang fp contract(off)" in core and "#pragma clang fp contract(off)" in unit
    assert re.search(r"^\$\(OBJ\)/rdoq\.o: FLAGS \+= -ffp-contract=off$", make, flags=re.M)
    assert "fast-math" not in make and "-ffast-math" not in unit
    assert "c_entropy_bits[128]" in tables and "c_entropy_bits[" in core and "c_entropy_bits[128] =" not in core
    assert "c_cc_group_idx[32]" in cabac and "c_cc_group_idx[" in core and "cc_sig_ctx_inc(" in core
    import rdoq_model as M
    numbers = [int(v, 16) for v in re.findall(r"0x[0-9a-f]{5}", tables[tables.index("c_entropy_bits[128]"):])]
    assert numbers == list(M.ENTROPY_BITS)

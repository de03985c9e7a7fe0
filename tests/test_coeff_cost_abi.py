"""CPU: the declarations of the CABAC coefficient pricing -- kvz_hip_coeff_cost_batch, kvz_hip_inter_residual_frame_ts_cabac and
kvz_hip_intra_recon_frame_ts_cabac declared, documented, exported and bound; kvz_hip_coeff_ctx, kvz_hip_coeff_cost_desc,
kvz_hip_coeff_cost_params and kvz_hip_coeff_pricing in C99, in ctypes / numpy and in the header's comments; the ABI
version unchanged; the argument checks of kvazaar_amd/csrc/coeff_cost_host.h as a host program; with a device every error path of the
three entries returns KVZ_HIP_ERR_INVALID and pricing == NULL / ts == NULL delegate (kvz_hip_last_error names the entry that refused),
without one the entries say so before they look at anything; the helper that cuts a record from a context dump."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_abi as A

ENTRY = "kvz_hip_coeff_cost_batch"
STAGES = ("kvz_hip_inter_residual_frame_ts_cabac", "kvz_hip_intra_recon_frame_ts_cabac")


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entry():
    L = _lib()
    from kvazaar_amd import _lib as B
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    assert ENTRY in A.declared_symbols() and hasattr(L, ENTRY) and hasattr(B.load(), ENTRY)
    assert re.search(r"\bT %s\b" % ENTRY, exported)
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert B.SIGNATURES[ENTRY] == (I, [P, P, ctypes.c_size_t, P, U, ctypes.POINTER(B.CoeffCostParams), P, P])
    for name in STAGES:
        assert name in A.declared_symbols() and hasattr(L, name) and re.search(r"\bT %s\b" % name, exported), name
        # the _ts entry's arguments with the pricing before params
        old, new = B.SIGNATURES[name[:-len("_cabac")]], B.SIGNATURES[name]
        assert new[0] == old[0] and new[1] == old[1][:-2] + [ctypes.POINTER(B.CoeffPricing)] + old[1][-2:], name
    text = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    for name in STAGES:
        params = [a.strip() for a in re.search(r"%s\((.*?)\);" % name, text, flags=re.S).group(1).replace("\n", " ").split(",")]
        assert params[-3:] == ["const kvz_hip_coeff_pricing *pricing", "const kvz_hip_inter_residual_params *params", "kvz_hip_stream s"], name


def test_structs_in_c99_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B, api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %d", sizeof(kvz_hip_coeff_ctx), sizeof(kvz_hip_coeff_cost_desc), sizeof(kvz_hip_coeff_cost_params),',
             '         KVZ_HIP_ABI_VERSION);', '  printf(" %zu", sizeof(kvz_hip_coeff_pricing));']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_coeff_pricing, %s));' % f for f in ("ctx_sets", "n_sets", "fast_limit", "lcu_ctx")]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_coeff_ctx, %s));' % f for f in ("range", "reserved", "ctx")]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_coeff_cost_desc, %s));' % f for f in ("offset", "width", "type", "scan_mode", "tr_skip", "ctx_index")]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_coeff_cost_params, %s));' % f for f in ("signhide", "trskip_enable", "lossless", "reserved")]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [144, 12, 16, 4] + [24, 0, 8, 12, 16] + [0, 2, 4] + [0, 4, 5, 6, 7, 8] + [0, 4, 8, 12]
    assert ctypes.sizeof(B.CoeffPricing) == 24 and [getattr(B.CoeffPricing, f).offset for f in ("ctx_sets", "n_sets", "fast_limit", "lcu_ctx")] == [0, 8, 12, 16]
    assert api.COEFF_CTX.itemsize == 144 and [api.COEFF_CTX.fields[f][1] for f in ("range", "reserved", "ctx")] == [0, 2, 4]
    assert api.COEFF_COST_DESC.itemsize == 12
    assert [api.COEFF_COST_DESC.fields[f][1] for f in ("offset", "width", "type", "scan_mode", "tr_skip", "ctx_index")] == [0, 4, 5, 6, 7, 8]
    assert ctypes.sizeof(B.CoeffCostParams) == 16 and [f for f, _ in B.CoeffCostParams._fields_] == ["signhide", "trskip_enable", "lossless", "reserved"]


def test_header_documents_the_entry_and_what_stays_out():
    text = open(A.HEADER).read()
    at = text.index("Coefficient pricing with CABAC")
    doc = text[at:text.index("Lossless coding in the picture chain", at)]
    for phrase in ("rdo.c:158-197", "rdo.c:208-222", "encode_coding_tree.c:49-345", "context.c:303-385", "cabac.c:91-282", "cfg.c:82", "256..510",
                   "cu_sig_coeff_group_model[0]", "cu_abs_model_chroma[1]", "transform_skip_model_luma", "0..125", "multiple of 4", "z-order",
                   "left untouched", "KVZ_HIP_ERR_INVALID", "n == 0", "kvz_hip_graph_begin", "ABI version stays 4", "search.c:300", "RDOQ",
                   "transform-tree flag bits", "private copy", "crypto", "rdo.c:214", "pricing == NULL", "n_sets - 1", "rdo.c:188-194",
                   "cfg.fast_residual_cost_limit", "one set index per LCU", "pricing != NULL with ts == NULL", "costs 0 bits", "_frames_ts entries"):
        assert phrase in doc, phrase
    # the _ts comment points at the new entries
    ts_doc = text[text.index("kvz_hip_inter_residual_frame_sl and kvz_hip_intra_recon_frame_sl with two more arguments"):at]
    assert "kvz_hip_inter_residual_frame_ts_cabac" in ts_doc and "kvz_hip_coeff_cost_batch" in ts_doc
    assert re.search(r"#define KVZ_HIP_ABI_VERSION 4\b", text)


def test_context_record_from_a_dump():
    from kvazaar_amd import api
    dump = np.arange(184, dtype=np.uint8)
    rec = api.coeff_ctx_from_dump(dump, 300)
    assert rec["range"] == 300 and rec["reserved"] == 0
    assert rec["ctx"][:136].tolist() == list(range(32, 168)) and rec["ctx"][136:].tolist() == [182, 183, 0, 0]
    assert api.coeff_ctx_from_dump(bytes(184), 256)["ctx"].sum() == 0
    for bad in (lambda: api.coeff_ctx_from_dump(dump[:183], 300), lambda: api.coeff_ctx_from_dump(dump, 255), lambda: api.coeff_ctx_from_dump(dump, 511)):
        with pytest.raises(ValueError):
            bad()
    # the record's layout is the model's reading of the reference's block
    import coeff_cabac_model as M
    assert (M.FIRST_USED, M.END_USED, M.TS_LUMA, M.TS_CHROMA, M.CTX_BYTES) == (32, 168, 182, 183, api.CABAC_CTX_BYTES)


def test_every_error_path_returns_invalid_or_no_device():
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    f = L.kvz_hip_coeff_cost_batch
    prm = B.CoeffCostParams(1, 1, 0, 0)
    p = ctypes.byref(prm)
    good = [0x1000, 0x2000, 1, 0x3000, 1, p, 0x4000, None]            # never launched: one argument is broken each time

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[("coeffs", "descs", "n", "ctx_sets", "n_sets", "params", "bits_out").index(k)] = v
        return f(*a)

    for broken in (dict(coeffs=None), dict(descs=None), dict(ctx_sets=None), dict(params=None), dict(bits_out=None), dict(n_sets=0),
                   dict(coeffs=0x1004), dict(descs=0x2002), dict(ctx_sets=0x3001), dict(bits_out=0x4002), dict(n=1 << 31)):
        assert call(**broken) == want, broken
        if have:
            assert ENTRY.encode() in L.kvz_hip_last_error()
    # nothing to do is not an error, whatever the pointers are
    assert f(None, None, 0, None, 0, None, None, None) == (0 if have else no_device)


def _stage_args(B, inter, **kw):
    """valid-looking arguments of a _ts_cabac entry (never launched: every call here is refused), one of them replaced"""
    P = ctypes.c_void_p
    src = B.RefPicture(0x10000, 0x20000, 0x30000, 64, 32, 64, 64)
    prm = (ctypes.c_int32 * 8)(27, 0, 0, 0, 1, 0, 0, 0)               # kvz_hip_inter_residual_params: qp 27, 4:2:0
    ts = B.TrSkip(18, 0, None)
    pricing = B.CoeffPricing(0x90000, 2, 0, None)
    for k, v in kw.pop("pricing_fields", {}).items():
        setattr(pricing, k, v)
    a = dict(src=ctypes.addressof(src), rec_y=0x40000, sy=64, rec_u=0x41000, rec_v=0x42000, sc=32, cus=0x50000, modes=0x51000, cy=0x60000, cu=0x61000,
             cv=0x62000, cbf=None, costs=None, lcu_qp=None, grid=None, tables=None, ts=ctypes.pointer(ts), skip=0x70000, pricing=ctypes.pointer(pricing),
             prm=ctypes.addressof(prm), s=None)
    a.update(kw)
    order = ["src", "rec_y", "sy", "rec_u", "rec_v", "sc", "cus"] + ([] if inter else ["modes"]) + ["cy", "cu", "cv", "cbf", "costs", "lcu_qp"] + \
        ([] if inter else ["grid"]) + ["tables", "ts", "skip", "pricing", "prm", "s"]
    return [a[k] for k in order], (src, prm, ts, pricing)


def test_the_stages_refuse_and_delegate():
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    have = torch.cuda.is_available()
    want = -2 if have else -1
    for inter, name in zip((True, False), STAGES):
        f = getattr(L, name)
        cases = (dict(ts=None), dict(pricing_fields=dict(ctx_sets=None)), dict(pricing_fields=dict(ctx_sets=0x90001)), dict(pricing_fields=dict(n_sets=0)),
                 dict(pricing_fields=dict(lcu_ctx=0x91001)), dict(skip=None), dict(prm=None))
        for broken in cases:
            args, keep = _stage_args(B, inter, **broken)
            assert f(*args) == want, (name, broken)
            if have:
                assert (L.kvz_hip_last_error() or b"").decode().startswith(name + ":"), (name, broken, L.kvz_hip_last_error())
        # pricing == NULL: the _ts entry refuses in its own name; ts == NULL as well: an entry behind it does (the _sl entry, which
        # without tables hands on to the entry without them)
        stem = name[:-len("_ts_cabac")]
        for broken, who in ((dict(pricing=None, skip=None), (stem + "_ts",)), (dict(pricing=None, ts=None, cus=None), (stem, stem + "_sl", stem + "_qp", stem + "_tiles"))):
            args, keep = _stage_args(B, inter, **broken)
            assert f(*args) == want, (name, broken)
            if have:
                assert (L.kvz_hip_last_error() or b"").decode().split(":")[0] in who, (name, broken, L.kvz_hip_last_error())


PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "kvz_hip.h"
#include "coeff_cost_host.h"

int main()
{
  const kvz_hip_coeff *c = (const kvz_hip_coeff *)0x1000;
  const kvz_hip_coeff_cost_desc *d = (const kvz_hip_coeff_cost_desc *)0x2000;
  const kvz_hip_coeff_ctx *s = (const kvz_hip_coeff_ctx *)0x3002;
  const uint32_t *b = (const uint32_t *)0x4000;
  kvz_hip_coeff_cost_params p = { 1, 1, 0, 0 };
  struct { const char *name; const char *why; } r[] = {
    { "clean", coeff_cost_batch_why(c, d, 5, s, 1, &p, b) },
    { "largest n", coeff_cost_batch_why(c, d, 0x7fffffffu, s, 1, &p, b) },
    { "coeffs null", coeff_cost_batch_why(nullptr, d, 5, s, 1, &p, b) },
    { "descs null", coeff_cost_batch_why(c, nullptr, 5, s, 1, &p, b) },
    { "sets null", coeff_cost_batch_why(c, d, 5, nullptr, 1, &p, b) },
    { "params null", coeff_cost_batch_why(c, d, 5, s, 1, nullptr, b) },
    { "bits null", coeff_cost_batch_why(c, d, 5, s, 1, &p, nullptr) },
    { "no sets", coeff_cost_batch_why(c, d, 5, s, 0, &p, b) },
    { "n too large", coeff_cost_batch_why(c, d, (size_t)1 << 31, s, 1, &p, b) },
    { "coeffs at 4", coeff_cost_batch_why((const kvz_hip_coeff *)0x1004, d, 5, s, 1, &p, b) },
    { "descs at 2", coeff_cost_batch_why(c, (const kvz_hip_coeff_cost_desc *)0x2002, 5, s, 1, &p, b) },
    { "sets at 1", coeff_cost_batch_why(c, d, 5, (const kvz_hip_coeff_ctx *)0x3001, 1, &p, b) },
    { "bits at 2", coeff_cost_batch_why(c, d, 5, s, 1, &p, (const uint32_t *)0x4002) },
    { "null before no sets", coeff_cost_batch_why(nullptr, d, 5, s, 0, &p, b) },
  };
  for (auto &e : r) printf("%s: %s\n", e.name, e.why ? e.why : "ok");
  kvz_hip_trskip ts = { 18, 0, nullptr };
  kvz_hip_coeff_pricing ok = { s, 3, 0, nullptr }, with_ctx = { s, 3, 30, (const uint16_t *)0x5002 }, no_sets = { nullptr, 3, 0, nullptr },
                        odd_sets = { (const kvz_hip_coeff_ctx *)0x3001, 3, 0, nullptr }, zero = { s, 0, 0, nullptr }, odd_ctx = { s, 3, 0, (const uint16_t *)0x5001 };
  struct { const char *name; const char *why; } q[] = {
    { "pricing clean", coeff_pricing_why(&ok, &ts) }, { "pricing with lcu_ctx", coeff_pricing_why(&with_ctx, &ts) },
    { "pricing without ts", coeff_pricing_why(&ok, nullptr) }, { "pricing sets null", coeff_pricing_why(&no_sets, &ts) },
    { "pricing sets at 1", coeff_pricing_why(&odd_sets, &ts) }, { "pricing no sets", coeff_pricing_why(&zero, &ts) },
    { "pricing lcu_ctx at 1", coeff_pricing_why(&odd_ctx, &ts) }, { "pricing ts before sets", coeff_pricing_why(&no_sets, nullptr) },
  };
  for (auto &e : q) printf("%s: %s\n", e.name, e.why ? e.why : "ok");
  return 0;
}
"""
NULL, SETS, COUNT = "a pointer is null", "n_sets is 0", "n above 2^31 - 1"
ALIGN = "coeffs not 8-byte, descs or bits_out not 4-byte or ctx_sets not 2-byte aligned"
EXPECTED = {"clean": "ok", "largest n": "ok", "coeffs null": NULL, "descs null": NULL, "sets null": NULL, "params null": NULL, "bits null": NULL,
            "no sets": SETS, "n too large": COUNT, "coeffs at 4": ALIGN, "descs at 2": ALIGN, "sets at 1": ALIGN, "bits at 2": ALIGN,
            "null before no sets": NULL, "pricing clean": "ok", "pricing with lcu_ctx": "ok", "pricing without ts": "pricing without ts",
            "pricing sets null": "ctx_sets is null or not 2-byte aligned", "pricing sets at 1": "ctx_sets is null or not 2-byte aligned",
            "pricing no sets": "n_sets is 0", "pricing lcu_ctx at 1": "lcu_ctx not 2-byte aligned", "pricing ts before sets": "pricing without ts"}


def test_argument_checks_as_a_host_program(tmp_path):
    """coeff_cost_host.h takes a plain C++17 compiler with kvz_hip.h alone: the checks compare pointers and never follow them"""
    src, exe = tmp_path / "coeff_checks.cpp", tmp_path / "coeff_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(A.ROOT, "include"), "-I", os.path.join(A.ROOT, "kvazaar_amd", "csrc"), str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    assert got == EXPECTED


def test_the_shared_tables_left_the_search_cost_model_as_it_was():
    """the CABAC tables moved to a header of their own; me_cost.h and the counter read the same two arrays"""
    csrc = os.path.join(A.ROOT, "kvazaar_amd", "csrc")
    tables, cost, core = (open(os.path.join(csrc, n)).read() for n in ("cabac_tables.h", "me_cost.h", "coeff_cabac_core.h"))
    assert "c_range_lps[64 * 4]" in tables and "c_trans_lps[64]" in tables
    for user in (cost, core):
        assert '#include "cabac_tables.h"' in user and "c_range_lps[64 * 4] =" not in user and "c_range_lps[" in user

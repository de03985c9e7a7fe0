"""CPU: the RDOQ model (tests/rdoq_model.py) against tests/golden/rdoq.npz -- results recorded from the compiled reference's own kvz_rdoq --
the census of decision classes, the deliberate errors, and, where the reference is compiled here, the model against kvz_rdoq on further
seeded TUs and the reference's own tables; and kvazaar_amd/csrc/rdoq_core.h, the arithmetic the kernels execute, compiled as a host program
against the same fixture."""
import collections
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rdoq_cases as K
import rdoq_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "rdoq.npz")
MIN_PER_CLASS = 4


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    d = {k: z[k] for k in z.files}
    d["cases"] = K.unpack(d["coeffs"], d["desc"])
    return d


def _model(fx, case, **kw):
    c, width, type_, scan, block_type, tr_depth, set_, cfg = case
    signhide, sl = fx["configs"][cfg]
    return M.rdoq(c.tolist(), width, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(fx["lambdas"][set_]), fx["dumps"][set_].tolist(),
                  fx["quant"][sl], fx["err_scale"][sl], int(signhide), **kw)


def _want(fx, i):
    o, w = int(fx["desc"][i][0]), int(fx["desc"][i][1])
    return fx["dest"][o:o + w * w].tolist()


def test_fixture_holds_the_cases_and_numbers_only(fx):
    coeffs, desc = K.pack(K.cases())
    assert (coeffs == fx["coeffs"]).all() and (desc == fx["desc"]).all()
    dumps, qps, lambdas = K.context_sets(fx["base_ctx"])
    assert (dumps == fx["dumps"]).all() and (qps == fx["qps"]).all() and (lambdas == fx["lambdas"]).all()
    assert (fx["configs"] == np.array(K.CONFIGS)).all()
    assert all(fx[k].dtype.kind in "iuf" for k in fx if k != "cases")
    assert os.path.getsize(FIXTURE) <= max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden")) if f != "rdoq.npz")
    # what the cases cover
    d = fx["desc"].astype(np.int64)
    assert set(d[:, 1]) == {4, 8, 16, 32} and set(d[:, 2]) == {0, 2} and set(d[d[:, 1] == 32][:, 2]) == {0}
    for width in (4, 8):
        assert set(d[d[:, 1] == width][:, 3]) == {0, 1, 2}
    assert set(d[d[:, 1] > 8][:, 3]) == {0} and set(d[:, 4]) == {1, 2} and set(d[:, 5]) == {0, 1, 2, 3} and set(d[:, 7]) == {0, 1, 2, 3}
    used = set(fx["qps"][d[:, 6]].tolist())
    assert min(used) == 4 and max(used) == 51 and any(q > 30 for q in fx["qps"][d[d[:, 2] == 2][:, 6]])
    # flat lists are flat, the default ones are not: error_scale differs inside a table
    at = M.table_offset(1, 0, 0)
    assert len(set(fx["err_scale"][0][at:at + 64])) == 1 and len(set(fx["err_scale"][1][at:at + 64])) > 8


def test_model_equals_the_recorded_reference_and_the_census_is_complete(fx):
    census = collections.Counter()
    for i, case in enumerate(fx["cases"]):
        got = _model(fx, case, census=census)                  # an entry read before it was written would raise UnwrittenRead here
        assert got == _want(fx, i), "TU %d: %r" % (i, case[1:])
    assert [census[k] for k in M.CLASSES] == fx["census"].tolist()
    short = {k: census[k] for k in M.CLASSES if census[k] < MIN_PER_CLASS}
    assert not short, short


def test_recorded_results_are_not_plain_rounding(fx):
    """a kernel that merely quantises cannot pass: most seeded TUs differ from round-to-nearest with the same tables"""
    differs = collections.Counter()
    total = collections.Counter()
    for i, (c, width, type_, scan, block_type, tr_depth, set_, cfg) in enumerate(fx["cases"][:sum(n for _, n in K.SEEDED)]):
        sl = fx["configs"][cfg][1]
        qps = M.scaled_qp(type_, int(fx["qps"][set_]))
        at = M.table_offset(width.bit_length() - 3, (0 if block_type == 1 else 3) + (1 if type_ else 0), qps % 6)
        q_bits = 14 + qps // 6 + 7 - (width.bit_length() - 1)
        level = (np.abs(c.astype(np.int64)) * fx["quant"][sl][at:at + c.size] + (1 << (q_bits - 1))) >> q_bits
        total[width] += 1
        differs[width] += int((np.where(c < 0, -level, level) != np.array(_want(fx, i))).any())
    for width in (4, 8, 16, 32):
        assert differs[width] * 4 >= total[width] * 3, (width, differs[width], total[width])


def test_the_poison_raises_on_every_use_as_a_number():
    u = M.UNWRITTEN
    for bad in (lambda: u + 1.0, lambda: 1.0 - u, lambda: u < 1.0, lambda: 3 * u, lambda: bool(u), lambda: 1 if u else 0, lambda: u == 0, lambda: abs(u),
                lambda: u >> 2, lambda: int(u), lambda: float(u), lambda: -u, lambda: 5 > u, lambda: [1, 2][u]):
        with pytest.raises(M.UnwrittenRead):
            bad()


@pytest.mark.parametrize("name", M.FORGETTABLE)
def test_a_write_left_out_is_noticed_where_the_entry_is_read(fx, name):
    """the model with one write deliberately left out raises on TUs of every width: the arrays are read through the poison, by arithmetic
    and by truth test (dest), so the fixture run above, which raises nothing, read no entry that was never written"""
    seen = set()
    for case in fx["cases"][::5]:
        if not case[0].any():
            continue
        try:
            out = _model(fx, case, forget=name)
        except M.UnwrittenRead:
            seen.add(case[1])
            continue
        assert not any(out), "a TU that codes a level never read its %s at the last position" % name
    assert seen == {4, 8, 16, 32}


@pytest.mark.parametrize("name", sorted(M.MUTANTS))
def test_each_deliberate_error_is_caught(fx, name):
    for i, case in enumerate(fx["cases"]):
        if _model(fx, case, mutant=name) != _want(fx, i):
            return
    pytest.fail("no stored TU notices: " + M.MUTANTS[name])


STUB = r"""
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
typedef uint8_t u8; typedef uint32_t u32; typedef int16_t i16; typedef int32_t i32;
#define __device__
#define __forceinline__ inline
#define __constant__ const
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __ffs(int x) { return __builtin_ffs(x); }
"""


def test_the_kernels_core_header_as_a_host_program_equals_the_fixture(fx, tmp_path):
    """rdoq_core.h holds all of the arithmetic and takes its memory through an accessor, so it runs on the CPU with the device words
    stubbed out; both layouts (a wave's TU, a lane's interleaved 4x4 TU) give the recorded results byte for byte"""
    csrc = os.path.join(ROOT, "kvazaar_amd", "csrc")
    for name in ("rdoq_core.h", "coeff_cabac_core.h", "cabac_tables.h"):
        shutil.copy(os.path.join(csrc, name), tmp_path / name)
    (tmp_path / "kvz_hip_internal.h").write_text(STUB)
    so = tmp_path / "librdoq_core_host.so"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I", str(tmp_path), os.path.join(HERE, "c_host", "rdoq_core_host.cpp"),
           "-o", str(so)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = ctypes.CDLL(str(so))
    L.rdoq_core_host.restype = None
    L.rdoq_core_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_double] + [ctypes.c_void_p] * 4 + [ctypes.c_int]
    for strided in (0, 1):
        for i, (c, width, type_, scan, block_type, tr_depth, set_, cfg) in enumerate(fx["cases"]):
            if strided and width != 4:
                continue
            signhide, sl = fx["configs"][cfg]
            dump = fx["dumps"][set_]
            ctx = np.ascontiguousarray(dump[32:168])
            state = np.ascontiguousarray(np.concatenate([dump[181:182], dump[16:24]]))
            qps = M.scaled_qp(type_, int(fx["qps"][set_]))
            at = M.table_offset(width.bit_length() - 3, (0 if block_type == 1 else 3) + (1 if type_ else 0), qps % 6)
            quant = np.ascontiguousarray(fx["quant"][sl][at:at + c.size])
            err = np.ascontiguousarray(fx["err_scale"][sl][at:at + c.size])
            c = np.ascontiguousarray(c)
            out = np.zeros(c.size, dtype=np.int16)
            L.rdoq_core_host(strided, c.ctypes.data, out.ctypes.data, width, type_, scan, block_type, tr_depth, int(fx["qps"][set_]),
                             float(fx["lambdas"][set_]), ctx.ctypes.data, state.ctypes.data, quant.ctypes.data, err.ctypes.data, int(signhide))
            assert out.tolist() == _want(fx, i), (strided, i)


def _ref():
    import ref_rdoq as R
    if not R.available():
        pytest.skip("the reference's sources or the compiled reference are not on this machine")
    return R


def test_model_equals_the_compiled_reference_on_further_tus(fx):
    R = _ref()
    n = 0
    for c, width, type_, scan, block_type, tr_depth, set_, cfg in K.extra_cases(77, per_width=(400, 350, 200, 50)):
        signhide, sl = fx["configs"][cfg]
        want = R.rdoq(c, width, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(fx["lambdas"][set_]), fx["dumps"][set_], int(signhide), int(sl))
        got = M.rdoq(c.tolist(), width, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(fx["lambdas"][set_]), fx["dumps"][set_].tolist(),
                     fx["quant"][sl], fx["err_scale"][sl], int(signhide))
        assert got == want.tolist(), (n, width, type_, scan, block_type, tr_depth, set_, cfg)
        n += 1
    assert n == 1000


def test_tables_and_contexts_are_the_references_own(fx):
    R = _ref()
    assert R.entropy_bits() == list(M.ENTROPY_BITS)
    assert R.ctx_offsets() == (M.ROOT_CBF, M.QT_CBF_LUMA, M.QT_CBF_CHROMA, 32)
    assert (K.base_contexts(R.init_contexts) == fx["base_ctx"]).all()
    for sl in (0, 1):
        quant, err = R.packed_tables(sl)
        assert (quant == fx["quant"][sl]).all() and (err == fx["err_scale"][sl]).all()
    # the recorded results are what the reference gives today
    for i in range(0, len(fx["cases"]), 7):
        c, width, type_, scan, block_type, tr_depth, set_, cfg = fx["cases"][i]
        signhide, sl = fx["configs"][cfg]
        got = R.rdoq(c, width, type_, scan, block_type, tr_depth, int(fx["qps"][set_]), float(fx["lambdas"][set_]), fx["dumps"][set_], int(signhide), int(sl))
        assert got.tolist() == _want(fx, i), i

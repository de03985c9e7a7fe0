"""CPU: chain_rdoq_why (kvazaar_amd/csrc/chain_host.h), the argument check of kvz_hip_inter_residual_frame_rdoq and
kvz_hip_intra_recon_frame_rdoq, as a host program: the header takes a plain C++17 compiler with kvz_hip.h alone, the check compares
pointers and follows none but the HOST record.  The order of the checks is part of the interface: it decides which reason a record with
two defects reports."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "kvz_hip.h"
#include "chain_host.h"

void kvzhip::set_error_msg(const char *) {}

static kvz_hip_rdoq_source good()
{
  kvz_hip_rdoq_source r = { (const kvz_hip_coeff_ctx *)0x4002, (const kvz_hip_rdoq_state *)0x5008, (const uint16_t *)0x6002,
                            { (const int32_t *)0x7010, (const double *)0x8008 }, 6, 0 };
  return r;
}

int main()
{
  struct { const char *name; kvz_hip_rdoq_source r; } c[16];
  int n = 0;
  auto add = [&](const char *name, kvz_hip_rdoq_source r) { c[n].name = name; c[n].r = r; ++n; };
  kvz_hip_rdoq_source r = good();
  add("clean", r);
  r = good(); r.lcu_ctx = nullptr; add("no lcu_ctx", r);
  r = good(); r.rdoq_skip = 1; r.n_sets = 1; add("skip, one set", r);
  r = good(); r.ctx_sets = nullptr; add("sets null", r);
  r = good(); r.states = nullptr; add("states null", r);
  r = good(); r.tables.quant = nullptr; add("quant null", r);
  r = good(); r.tables.err_scale = nullptr; add("err null", r);
  r = good(); r.n_sets = 0; add("no sets", r);
  r = good(); r.ctx_sets = (const kvz_hip_coeff_ctx *)0x4001; add("sets at 1", r);
  r = good(); r.lcu_ctx = (const uint16_t *)0x6001; add("lcu_ctx at 1", r);
  r = good(); r.states = (const kvz_hip_rdoq_state *)0x5004; add("states at 4", r);
  r = good(); r.tables.err_scale = (const double *)0x8004; add("err at 4", r);
  r = good(); r.tables.quant = (const int32_t *)0x7008; add("quant at 8", r);
  r = good(); r.states = nullptr; r.n_sets = 0; add("null before no sets", r);
  r = good(); r.tables.quant = nullptr; r.ctx_sets = (const kvz_hip_coeff_ctx *)0x4001; add("table before alignment", r);
  r = good(); r.n_sets = 0; r.tables.quant = (const int32_t *)0x7008; add("no sets before alignment", r);
  for (int i = 0; i < n; ++i) {
    const char *why = chain_rdoq_why(&c[i].r);
    printf("%s: %s\n", c[i].name, why ? why : "ok");
  }
  return 0;
}
"""
NULL, TABLE, SETS = "ctx_sets or states is null", "a table is null", "n_sets is 0"
ALIGN2, ALIGN8, ALIGN16 = "ctx_sets or lcu_ctx not 2-byte aligned", "states or err_scale not 8-byte aligned", "quant not 16-byte aligned"
EXPECTED = {"clean": "ok", "no lcu_ctx": "ok", "skip, one set": "ok", "sets null": NULL, "states null": NULL, "quant null": TABLE, "err null": TABLE,
            "no sets": SETS, "sets at 1": ALIGN2, "lcu_ctx at 1": ALIGN2, "states at 4": ALIGN8, "err at 4": ALIGN8, "quant at 8": ALIGN16,
            "null before no sets": NULL, "table before alignment": TABLE, "no sets before alignment": SETS}


def test_chain_rdoq_why_as_a_host_program(tmp_path):
    src, exe = tmp_path / "rdoq_chain_checks.cpp", tmp_path / "rdoq_chain_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"),
           str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    assert got == EXPECTED


def test_both_entries_ask_the_predicate_and_report_it():
    csrc = os.path.join(ROOT, "kvazaar_amd", "csrc")
    for unit in ("inter_residual_rdoq.hip", "intra_recon_rdoq.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "chain_rdoq_why(rdoq)" in text and "refuse_entry(__func__" in text, unit

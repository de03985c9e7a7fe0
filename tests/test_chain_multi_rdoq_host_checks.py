"""CPU: the record checks of kvz_hip_inter_residual_frames_rdoq and kvz_hip_intra_recon_frames_rdoq (chain_record_rdoq_why and
chain_record_rdoq_shared, kvazaar_amd/csrc/chain_host.h) as a host program: the header takes a plain C++17 compiler with kvz_hip.h
alone.  The program calls the walk that the entries call (chain_records_why) -- homogeneity and the record's own checks, for the intra
entry the grid and its place in the pool, the outputs of the earlier records -- and prints the first record that is refused with its
reason.  The order of the checks is part of the interface: it decides which reason a record with two defects reports.

The walk also returns what the records ask of the launches (chain_plan): the program prints it for the smallest calls at which each
term can be wrong, for the three record types.  The expected figures follow from the rules, not from the code: a tile of w x h LCUs
takes w + 2 (h - 1) dependent launches, a picture a workgroup per LCU row and tile column, the init launch the SCUs of the largest
picture that has cbf_out or costs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "kvz_hip.h"
#include "chain_host.h"

void kvzhip::set_error_msg(const char *) {}

static kvz_hip_rdoq_source source()
{
  kvz_hip_rdoq_source r = { (const kvz_hip_coeff_ctx *)0x4002, (const kvz_hip_rdoq_state *)0x5008, (const uint16_t *)0x6002,
                            { (const int32_t *)0x7010, (const double *)0x8008 }, 6, 0 };
  return r;
}

// four records of 128 x 64 pictures with chroma, flat lists, apart from each other; each with a source of its own
struct call {
  kvz_hip_chain_picture_rdoq rec[16];
  kvz_hip_rdoq_source rq[16];
  kvz_hip_tile_grid grid[16];
  int n;
};

static void good(call &c, int n, int width = 128, int height = 64)
{
  memset(&c, 0, sizeof c);
  c.n = n;
  for (int i = 0; i < n; ++i) {
    kvz_hip_chain_picture &p = c.rec[i].pic;
    const uintptr_t at = 0x1000000u * (uintptr_t)(i + 1);
    p.src.y = (const kvz_hip_pixel *)(at + 0x100000); p.src.u = (const kvz_hip_pixel *)(at + 0x200000); p.src.v = (const kvz_hip_pixel *)(at + 0x300000);
    p.src.stride_y = (uint32_t)width; p.src.stride_c = (uint32_t)width / 2; p.src.width = width; p.src.height = height;
    p.rec_y = (kvz_hip_pixel *)(at + 0x400000); p.rec_u = (kvz_hip_pixel *)(at + 0x500000); p.rec_v = (kvz_hip_pixel *)(at + 0x600000);
    p.stride_y = (uint32_t)width; p.stride_c = (uint32_t)width / 2;
    p.cus = (kvz_hip_cu_info *)(at + 0x700000); p.intra_modes = (const uint8_t *)(at + 0x800000);
    p.coeff_y = (kvz_hip_coeff *)(at + 0x900000); p.coeff_u = (kvz_hip_coeff *)(at + 0xa00000); p.coeff_v = (kvz_hip_coeff *)(at + 0xb00000);
    p.params.qp = 27; p.params.chroma = 1;
    c.rq[i] = source();
    c.rec[i].rdoq = &c.rq[i];
  }
}

static void tables(call &c, int i)
{
  c.rec[i].tables.quant = (const int32_t *)0x9010; c.rec[i].tables.dequant = (const int32_t *)0x9810;
  c.rec[i].pic.params.scaling_list = 1;
}

// cols x rows tiles of a picture of lx x ly LCUs
static void grid(call &c, int i, int cols, int rows, int lx, int ly)
{
  kvz_hip_tile_grid &g = c.grid[i];
  g.cols = cols; g.rows = rows;
  for (int j = 0; j <= cols; ++j) g.col_bd[j] = j * lx / cols;
  for (int j = 0; j <= rows; ++j) g.row_bd[j] = j * ly / rows;
  c.rec[i].grid = &g;
}

// record i becomes a picture of another size
static void size(call &c, int i, int width, int height)
{
  kvz_hip_chain_picture &p = c.rec[i].pic;
  p.src.width = width; p.src.height = height;
  p.src.stride_y = p.stride_y = (uint32_t)width; p.src.stride_c = p.stride_c = (uint32_t)width / 2;
}

// the call through the walk that the entries make (chain_records_why, chain_host.h), which alone decides the order of the checks; the
// inter entry never looks at a grid
static void report(const char *name, const call &c, bool intra)
{
  chain_tiles tiles;
  chain_plan plan;
  int at = -1;
  const char *why = chain_records_why(c.rec, c.n, intra, intra ? &tiles : nullptr, &plan, &at);
  if (why) printf("%s: picture %d: %s\n", name, at, why);
  else printf("%s: ok\n", name);
}

// what the walk says the records ask of the launches; the call is accepted
template <typename RECORD>
static void plan_of(const char *name, const RECORD *rec, int n, bool intra)
{
  chain_tiles tiles;
  chain_plan plan;
  int at = -1;
  const char *why = chain_records_why(rec, n, intra, intra ? &tiles : nullptr, &plan, &at);
  if (why) printf("plan %s: picture %d: %s\n", name, at, why);
  else printf("plan %s: waves %d groups %d planes %d init_scus %d\n", name, plan.waves, plan.groups, plan.planes, plan.init_scus);
}

static void plans()
{
  static call c;
  good(c, 4); plan_of("four untiled 128x64", c.rec, c.n, true);
  good(c, 4); grid(c, 1, 2, 1, 2, 1); plan_of("2x1 tiles in record 1", c.rec, c.n, true);
  good(c, 2); size(c, 0, 1024, 512); grid(c, 0, 16, 8, 16, 8); plan_of("16x8 tiles of one LCU beside untiled 128x64", c.rec, c.n, true);
  good(c, 1, 1024, 512); plan_of("untiled 1024x512", c.rec, c.n, true);
  good(c, 3); for (int i = 0; i < 3; ++i) c.rec[i].pic.params.chroma = 0;
  plan_of("4:0:0 only", c.rec, c.n, true);
  good(c, 3); c.rec[0].pic.params.chroma = 0; c.rec[2].pic.params.chroma = 0; plan_of("4:2:0 among 4:0:0", c.rec, c.n, true);
  good(c, 3); size(c, 0, 1024, 512); size(c, 2, 1920, 1080); c.rec[1].pic.costs = (kvz_hip_inter_residual_cost *)0x3000;
  plan_of("costs on the 128x64 record alone", c.rec, c.n, true);
  plan_of("costs on the 128x64 record alone, inter", c.rec, c.n, false);
  good(c, 3); size(c, 0, 1024, 512); c.rec[0].pic.cbf_out = (uint8_t *)0x3000; c.rec[1].pic.costs = (kvz_hip_inter_residual_cost *)0x4000;
  plan_of("cbf_out on 1024x512 beside costs on 128x64", c.rec, c.n, true);
  // kvz_hip_intra_recon_frames and kvz_hip_intra_recon_frames_ts go through the same code: the embedded pictures as records that have
  // no grid (one tile each), and as records that carry the grids
  good(c, 2); size(c, 0, 1024, 512); grid(c, 0, 16, 8, 16, 8);
  kvz_hip_chain_picture plain[2] = { c.rec[0].pic, c.rec[1].pic };
  kvz_hip_chain_picture_ts ts[2];
  static kvz_hip_trskip skip = { 5, 0, nullptr };
  for (int i = 0; i < 2; ++i) ts[i] = { c.rec[i].pic, c.rec[i].grid, c.rec[i].tables, &skip, (uint8_t *)(uintptr_t)(0x5000 + 0x1000 * i) };
  plan_of("plain records, 1024x512 and 128x64", plain, 2, true);
  plan_of("ts records, 1024x512 in 16x8 tiles and 128x64", ts, 2, true);
}

int main()
{
  static call c;
  good(c, 4); report("clean", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) tables(c, i);
  report("clean with tables", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) c.rq[i].rdoq_skip = 1 + i;     // any non-zero value is "skip"
  report("clean with skip", c, false);
  good(c, 3); c.rq[1].ctx_sets = (const kvz_hip_coeff_ctx *)0x14002; c.rq[1].states = (const kvz_hip_rdoq_state *)0x15008; c.rq[1].lcu_ctx = nullptr; c.rq[1].n_sets = 1;
  report("own sets per picture", c, true);
  good(c, 4); grid(c, 1, 2, 1, 2, 1);
  report("tiled beside untiled", c, true);

  // each refusal of the single entry's rdoq check, at the record that has it
  good(c, 4); c.rq[2].ctx_sets = nullptr; report("sets null", c, true);
  good(c, 4); c.rq[3].states = nullptr; report("states null", c, false);
  good(c, 4); c.rq[1].n_sets = 0; report("no sets", c, true);
  good(c, 4); c.rq[1].ctx_sets = (const kvz_hip_coeff_ctx *)0x4001; report("sets at 1", c, true);
  good(c, 4); c.rq[2].lcu_ctx = (const uint16_t *)0x6001; report("lcu_ctx at 1", c, false);
  good(c, 4); c.rq[3].states = (const kvz_hip_rdoq_state *)0x5004; report("states at 4", c, true);
  // the shared tables are record 0's: a defect of theirs shows at record 0, whose own checks come first
  good(c, 4); for (int i = 0; i < 4; ++i) c.rq[i].tables.quant = nullptr;
  report("quant null", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) c.rq[i].tables.err_scale = (const double *)0x8004;
  report("err at 4", c, false);
  good(c, 4); for (int i = 0; i < 4; ++i) c.rq[i].tables.quant = (const int32_t *)0x7008;
  report("quant at 8", c, true);
  // the record's own checks
  good(c, 4); c.rec[2].pic.cus = nullptr; report("cus null", c, true);
  good(c, 4); c.rec[1].pic.intra_modes = nullptr; report("modes null, intra", c, true);
  good(c, 4); c.rec[1].pic.intra_modes = nullptr; report("modes null, inter", c, false);
  good(c, 4); c.rec[3].pic.params.qp = -1; report("negative qp", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) tables(c, i);
  c.rec[2].tables.dequant = (const int32_t *)0x9818; report("table at 8", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) tables(c, i);
  c.rec[1].pic.params.scaling_list = 0; report("tables without scaling_list", c, false);
  good(c, 4); c.rec[2].pic.params.scaling_list = 1; report("scaling_list without tables", c, true);
  good(c, 4); grid(c, 2, 2, 1, 3, 1); report("grid of another width", c, true);
  good(c, 4); grid(c, 2, 2, 1, 3, 1); report("grid of another width, inter", c, false);
  good(c, 4); c.rec[3].pic.rec_y = c.rec[1].pic.rec_y; report("shared rec_y", c, true);
  good(c, 4); c.rec[2].pic.cus = c.rec[0].pic.cus; report("shared cus", c, false);
  good(c, 4); c.rec[1].pic.coeff_y = c.rec[0].pic.coeff_y; report("shared coeff_y", c, true);

  // homogeneity: the five shared properties, each way round where there are two
  good(c, 4); tables(c, 2); report("tables among none", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) tables(c, i);
  c.rec[1].tables.quant = c.rec[1].tables.dequant = nullptr; c.rec[1].pic.params.scaling_list = 0; report("none among tables", c, false);
  good(c, 4); c.rec[2].rdoq = nullptr; report("no rdoq among rdoq", c, true);
  good(c, 4); c.rec[0].rdoq = nullptr; report("rdoq after a record 0 without", c, false);
  good(c, 4); c.rq[3].rdoq_skip = 1; report("skip among no skip", c, true);
  good(c, 4); for (int i = 0; i < 4; ++i) c.rq[i].rdoq_skip = 1;
  c.rq[1].rdoq_skip = 0; report("no skip among skip", c, false);
  good(c, 4); c.rq[2].tables.quant = (const int32_t *)0x17010; report("another quant", c, true);
  good(c, 4); c.rq[1].tables.err_scale = (const double *)0x18008; report("another err_scale", c, false);

  // two defects: homogeneity before the record's own checks, those before the grid, the grid before the earlier records' outputs; and
  // the first refused record is the one that is named
  good(c, 4); c.rq[2].rdoq_skip = 1; c.rq[2].ctx_sets = nullptr; report("skip differs and sets null", c, true);
  good(c, 4); c.rq[2].tables.quant = nullptr; report("quant null in one record", c, true);
  good(c, 4); tables(c, 1); c.rec[1].tables.dequant = nullptr; c.rec[1].pic.cus = nullptr; report("half tables among none and cus null", c, true);
  good(c, 4); c.rec[2].pic.cus = nullptr; c.rq[2].n_sets = 0; report("cus null and no sets", c, true);
  good(c, 4); c.rq[2].n_sets = 0; c.rec[2].pic.params.qp = -1; report("no sets and negative qp", c, true);
  good(c, 4); c.rec[2].pic.params.qp = -1; grid(c, 2, 2, 1, 3, 1); report("negative qp and bad grid", c, true);
  good(c, 4); grid(c, 2, 2, 1, 3, 1); c.rec[2].pic.rec_y = c.rec[0].pic.rec_y; report("bad grid and shared rec_y", c, true);
  good(c, 4); c.rec[3].pic.cus = nullptr; c.rec[1].pic.rec_y = c.rec[0].pic.rec_y; report("shared at 1 and cus null at 3", c, true);

  // the pool: 1024 x 512 pictures are 16 x 8 LCUs; 16 x 8 tiles take 26 boundaries.  9 x 26 + 22 = 256 fit; 9 x 26 + 19 + 4 = 257 do not,
  // at the record where it overflows; records without a grid take nothing
  good(c, 12, 1024, 512); for (int i = 0; i < 9; ++i) grid(c, i, 16, 8, 16, 8);
  grid(c, 9, 12, 8, 16, 8); report("pool exactly full", c, true);
  good(c, 12, 1024, 512); for (int i = 0; i < 9; ++i) grid(c, i, 16, 8, 16, 8);
  grid(c, 9, 9, 8, 16, 8); grid(c, 11, 1, 1, 16, 8); report("pool overflows at 11", c, true);
  good(c, 12, 1024, 512); for (int i = 0; i < 9; ++i) grid(c, i, 16, 8, 16, 8);
  grid(c, 9, 9, 8, 16, 8); grid(c, 11, 1, 1, 16, 8); report("no pool in the inter entry", c, false);
  good(c, 12, 1024, 512); for (int i = 0; i < 10; ++i) grid(c, i, 16, 8, 16, 8);
  c.rec[9].pic.rec_y = c.rec[0].pic.rec_y; report("pool before shared outputs", c, true);
  plans();
  return 0;
}
"""
HOMOGENEOUS = "a call is homogeneous: every record carries tables or none does, every record carries rdoq or none does"
SAME = "a call is homogeneous: rdoq_skip, rdoq->tables.quant and rdoq->tables.err_scale are those of record 0"
ARGS = "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given"
TABLE = "a table is null or not 16-byte aligned"
SHARED = "an output shared with another picture"
POOL = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record"
EXPECTED = {
    "clean": "ok", "clean with tables": "ok", "clean with skip": "ok", "own sets per picture": "ok", "tiled beside untiled": "ok",
    "sets null": "picture 2: ctx_sets or states is null", "states null": "picture 3: ctx_sets or states is null", "no sets": "picture 1: n_sets is 0",
    "sets at 1": "picture 1: ctx_sets or lcu_ctx not 2-byte aligned", "lcu_ctx at 1": "picture 2: ctx_sets or lcu_ctx not 2-byte aligned",
    "states at 4": "picture 3: states or err_scale not 8-byte aligned", "quant null": "picture 0: a table is null",
    "err at 4": "picture 0: states or err_scale not 8-byte aligned", "quant at 8": "picture 0: quant not 16-byte aligned",
    "cus null": "picture 2: " + ARGS, "modes null, intra": "picture 1: " + ARGS, "modes null, inter": "ok", "negative qp": "picture 3: a negative qp without lcu_qp",
    "table at 8": "picture 2: " + TABLE, "tables without scaling_list": "picture 1: " + ARGS, "scaling_list without tables": "picture 2: " + ARGS,
    "grid of another width": "picture 2: invalid tile grid", "grid of another width, inter": "ok",
    "shared rec_y": "picture 3: " + SHARED, "shared cus": "picture 2: " + SHARED, "shared coeff_y": "picture 1: " + SHARED,
    "tables among none": "picture 2: " + HOMOGENEOUS, "none among tables": "picture 1: " + HOMOGENEOUS, "no rdoq among rdoq": "picture 2: " + HOMOGENEOUS,
    "rdoq after a record 0 without": "picture 1: " + HOMOGENEOUS, "skip among no skip": "picture 3: " + SAME, "no skip among skip": "picture 1: " + SAME,
    "another quant": "picture 2: " + SAME, "another err_scale": "picture 1: " + SAME,
    "skip differs and sets null": "picture 2: " + SAME, "quant null in one record": "picture 2: " + SAME,
    "half tables among none and cus null": "picture 1: " + HOMOGENEOUS, "cus null and no sets": "picture 2: " + ARGS,
    "no sets and negative qp": "picture 2: n_sets is 0", "negative qp and bad grid": "picture 2: a negative qp without lcu_qp",
    "bad grid and shared rec_y": "picture 2: invalid tile grid", "shared at 1 and cus null at 3": "picture 1: " + SHARED,
    "pool exactly full": "ok", "pool overflows at 11": "picture 11: " + POOL, "no pool in the inter entry": "ok", "pool before shared outputs": "picture 9: " + POOL,
}


# what the records ask of the launches: "waves groups planes init_scus".  128 x 64 is 2 x 1 LCUs (2 waves, 1 workgroup), 1024 x 512 is
# 16 x 8 (16 + 2 * 7 = 30 waves, 8 workgroups), 1920 x 1080 is 30 x 17 (30 + 2 * 16 = 62, 17)
EXPECTED_PLAN = {
    "four untiled 128x64": (2, 1, 3, 0),
    "2x1 tiles in record 1": (2, 2, 3, 0),                              # its tiles are one LCU, one wave: the untiled records' 2 stand
    "16x8 tiles of one LCU beside untiled 128x64": (2, 8 * 16, 3, 0),
    "untiled 1024x512": (30, 8, 3, 0),
    "4:0:0 only": (2, 1, 1, 0),
    "4:2:0 among 4:0:0": (2, 1, 3, 0),
    "costs on the 128x64 record alone": (62, 17, 3, 32 * 16),
    "costs on the 128x64 record alone, inter": (0, 0, 1, 32 * 16),      # the inter stage sizes its launches of the kernel's records
    "cbf_out on 1024x512 beside costs on 128x64": (30, 8, 3, 256 * 128),
    "plain records, 1024x512 and 128x64": (30, 8, 3, 0),
    "ts records, 1024x512 in 16x8 tiles and 128x64": (2, 8 * 16, 3, 0),
}


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    """the program's lines, compiled and run once for the module: ({case: verdict}, {case: plan})"""
    tmp = tmp_path_factory.mktemp("multi_rdoq_checks")
    src, exe = tmp / "multi_rdoq_checks.cpp", tmp / "multi_rdoq_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"),
           str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    plans = {name[len("plan "):]: got.pop(name) for name in list(got) if name.startswith("plan ")}
    return got, plans


def test_record_checks_as_a_host_program(program_output):
    got, _ = program_output
    assert got == EXPECTED


def test_the_walk_returns_the_launch_plan(program_output):
    _, plans = program_output
    assert plans == {name: "waves %d groups %d planes %d init_scus %d" % plan for name, plan in EXPECTED_PLAN.items()}


UNITS = ("inter_residual_multi.hip", "inter_residual_multi_ts.hip", "inter_residual_multi_rdoq.hip",
         "intra_recon_multi.hip", "intra_recon_multi_ts.hip", "intra_recon_multi_rdoq.hip")


def test_the_six_entries_call_the_walk_and_spell_no_check_themselves():
    """the order of the checks is executed above; what is left to pin in text is that the entries call what was executed, refuse with
    what it returned before they launch anything, and check nothing beside it"""
    import re
    csrc = os.path.join(ROOT, "kvazaar_amd", "csrc")
    for unit in UNITS:
        text = open(os.path.join(csrc, unit)).read()
        intra = "true, &tiles" if unit.startswith("intra") else "false, nullptr"
        call = "if (const char *why = chain_records_why(pictures, n_pictures, %s, &plan, &at)) return refuse_picture(__func__, at, why);" % intra
        assert text.count("chain_records_why(") == 1 and text.count(call) == 1, unit
        # the entry launches nothing before the walk: neither itself nor through a helper of its unit
        entry = text[text.index('extern "C" {'):]
        before = entry[:entry.index(call)]
        assert "hipLaunchKernelGGL(" not in before and "launch_" not in before and "init_pictures" not in before and "ctx_stream(" not in before, unit
        for gone in (r"tile_pool_add\(", r"tile_grid_make\(", r"chain_record_\w*why\(", r"chain_record_\w*shared\(", r"chain_picture_args_ok\("):
            assert not re.search(gone, text), (unit, gone)

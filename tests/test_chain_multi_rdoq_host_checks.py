"""CPU: the record checks of kvz_hip_inter_residual_frames_rdoq and kvz_hip_intra_recon_frames_rdoq (chain_record_rdoq_why and
chain_record_rdoq_shared, kvazaar_amd/csrc/chain_host.h) as a host program: the header takes a plain C++17 compiler with kvz_hip.h
alone.  The program walks the records as the intra entry does -- homogeneity and the record's own checks, the grid and its place in the
pool, the outputs of the earlier records -- and prints the first record that is refused with its reason.  The order of the checks is
part of the interface: it decides which reason a record with two defects reports."""
import os
import subprocess

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

// the checks of a call in the order of the intra entry (intra_recon_multi_rdoq.hip); the inter entry leaves the grid out
static void report(const char *name, const call &c, bool intra)
{
  const kvz_hip_rdoq_source *first = c.rec[0].rdoq;
  const bool lists = c.rec[0].tables.quant || c.rec[0].tables.dequant, skip = first && first->rdoq_skip != 0;
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  int used = 0;
  for (int i = 0; i < c.n; ++i) {
    const char *why = chain_record_rdoq_why(c.rec, i, intra, lists, skip);
    kvz_hip_tile_grid g;
    pic_tiles t;
    if (intra && !why && !tile_grid_make(c.rec[i].grid, c.rec[i].pic.src.width, c.rec[i].pic.src.height, &g)) why = "invalid tile grid";
    if (intra && !why && !tile_pool_add(c.rec[i].grid, g, bounds, used, &t)) why = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record";
    if (!why) why = chain_record_rdoq_shared(c.rec, i);
    if (why) { printf("%s: picture %d: %s\n", name, i, why); return; }
  }
  printf("%s: ok\n", name);
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


def test_record_checks_as_a_host_program(tmp_path):
    src, exe = tmp_path / "multi_rdoq_checks.cpp", tmp_path / "multi_rdoq_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"),
           str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    assert got == EXPECTED


def test_both_entries_walk_the_records_in_that_order():
    csrc = os.path.join(ROOT, "kvazaar_amd", "csrc")
    intra = open(os.path.join(csrc, "intra_recon_multi_rdoq.hip")).read()
    intra = intra[intra.index("int kvz_hip_intra_recon_frames_rdoq("):]
    at = [intra.index(s) for s in ("chain_record_rdoq_why(pictures, i, true, lists, skip)", "tile_grid_make(r.grid", "tile_pool_add(r.grid",
                                   "chain_record_rdoq_shared(pictures, i)", "refuse_picture(__func__, i, why)", "hipLaunchKernelGGL(")]
    assert at == sorted(at)
    inter = open(os.path.join(csrc, "inter_residual_multi_rdoq.hip")).read()
    body = inter[inter.index("int kvz_hip_inter_residual_frames_rdoq("):]
    at = [body.index(s) for s in ("chain_record_rdoq_why(pictures, i, false, lists, skip)", "chain_record_rdoq_shared(pictures, i)",
                                  "refuse_picture(__func__, i, why)", "hipLaunchKernelGGL(")]
    assert at == sorted(at) and "tile_grid_make" not in inter

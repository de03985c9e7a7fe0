"""CPU: the record checks of the multi-picture residual entries (kvazaar_amd/csrc/chain_host.h) without a device.

Every kvz_hip_*_frames entry returns KVZ_HIP_ERR_NO_DEVICE before it looks at a record, so on a machine without a GPU nothing ever ran
these checks.  They are pointer and integer arithmetic on the structs of kvz_hip.h: a stand-alone C++ program includes the header with
kvz_hip.h alone, builds records on fake, suitably aligned pointer values (the checks compare pointers and never follow them; only a
kvz_hip_tile_grid and a kvz_hip_trskip are read, and those are host memory) and prints, per case, the index of the first refused record
and its reason.  It is compiled with the address and undefined-behaviour sanitizers, their runtimes linked statically so that the
program does not depend on what else the process has loaded, and run as a child process.

The expected indices of the defects that tests/test_gpu_chain_multi.py and tests/test_gpu_chain_multi_ts.py plant are the ones those tests
assert; the expected reasons are the message strings of the entries as they stood before the checks moved into the header, copied here
as literals.

The same program runs the named checks of the options -- tables, the transform-skip source with its output, the one-QP rule -- which
the single-picture entries and the record checks share, and the packing of a single-picture entry's loose arguments into a record.
The one-QP rule is held against what make_consts (quant_core.h, which this program cannot include) decided for the probe that the
tiled intra entries used to make, make_consts(4, 0, 0) and make_consts(4, 2, 2): a host program that includes quant_core.h printed
that table once for every QP in -64..127, intra and inter slices, with and without sign hiding: refused below 0, accepted from 0."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reasons, as the four entries spelled them
PLAIN = "null or misaligned buffer, size or parameter out of range, or an output shared with another picture"
HOMOGENEOUS = "a call is homogeneous: every record carries tables or none does, every record carries ts or none does"
TABLE = "a table is null or not 16-byte aligned"
ARGS = "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given"
TS = "ts without tr_skip_out, a negative bit_cost without lcu_bit_cost, or a misaligned lcu_bit_cost"
QP = "a negative qp without lcu_qp"
GRID = "invalid tile grid"
POOL = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record"
SHARED = "an output shared with another picture"

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <string>

#include "kvz_hip.h"
#include "chain_host.h"

static std::string last_message;
void kvzhip::set_error_msg(const char *what) { last_message = what; }

// a pointer value that nothing is ever read through: slot k of record i, 4 KB apart
template <typename T> static T *fake(int i, int k) { return (T *)(uintptr_t)(0x10000000u + 0x100000u * (unsigned)i + 0x1000u * (unsigned)k); }

static kvz_hip_trskip skip_by_cost = { 5, 0, nullptr };
enum { MAX = KVZ_HIP_MAX_CHAIN_PICTURES };

// record i of a clean call: 64x64 and 8x8 in turn, 4:2:0, every optional output given
static kvz_hip_chain_picture clean(int i)
{
  const int size = i % 2 ? 8 : 64;
  kvz_hip_chain_picture p;
  memset(&p, 0, sizeof p);
  p.src.y = fake<kvz_hip_pixel>(i, 0); p.src.u = fake<kvz_hip_pixel>(i, 1); p.src.v = fake<kvz_hip_pixel>(i, 2);
  p.src.stride_y = (uint32_t)size; p.src.stride_c = (uint32_t)size / 2; p.src.width = p.src.height = size;
  p.rec_y = fake<kvz_hip_pixel>(i, 3); p.rec_u = fake<kvz_hip_pixel>(i, 4); p.rec_v = fake<kvz_hip_pixel>(i, 5);
  p.stride_y = (uint32_t)size; p.stride_c = (uint32_t)size / 2;
  p.cus = fake<kvz_hip_cu_info>(i, 6); p.intra_modes = fake<uint8_t>(i, 7);
  p.coeff_y = fake<kvz_hip_coeff>(i, 8); p.coeff_u = fake<kvz_hip_coeff>(i, 9); p.coeff_v = fake<kvz_hip_coeff>(i, 10);
  p.cbf_out = fake<uint8_t>(i, 11); p.costs = fake<kvz_hip_inter_residual_cost>(i, 12);
  p.params.qp = 30; p.params.chroma = 1;
  return p;
}
static kvz_hip_chain_picture_ts clean_ts(int i, bool lists, bool skip)
{
  kvz_hip_chain_picture_ts r;
  memset(&r, 0, sizeof r);
  r.pic = clean(i);
  if (lists) { r.tables.quant = fake<int32_t>(i, 13); r.tables.dequant = fake<int32_t>(i, 14); r.pic.params.scaling_list = 1; }
  if (skip) { r.ts = &skip_by_cost; r.tr_skip_out = fake<uint8_t>(i, 15); }
  return r;
}

// n records as a call of the inter and of the intra entry of their type: the walk that the entries make (chain_records_why), which
// alone decides the order of the checks.  The intra entry alone reads the grid
template <typename RECORD>
static void report(const char *name, int n, const RECORD *r)
{
  for (int intra = 0; intra < 2; ++intra) {
    const char *stage = intra ? "intra" : "inter";
    chain_tiles tiles;
    chain_plan plan;
    int at = -1;
    const char *w = chain_records_why(r, n, intra != 0, intra ? &tiles : nullptr, &plan, &at);
    if (!w) { printf("%s/%s: ok\n", name, stage); continue; }
    // through refuse_picture, as the entries do: the message names the record
    refuse_picture("entry", at, w);
    char head[64];
    snprintf(head, sizeof head, "entry: invalid argument in picture %d (", at);
    if (last_message != std::string(head) + w + ")") printf("%s/%s: MESSAGE %s\n", name, stage, last_message.c_str());
    else printf("%s/%s: %d %s\n", name, stage, at, w);
  }
}

// kvz_hip_inter_residual_frames / kvz_hip_intra_recon_frames on n records that `plant` changed
static void plain_case(const char *name, int n, const std::function<void(kvz_hip_chain_picture *)> &plant)
{
  kvz_hip_chain_picture p[MAX];
  for (int i = 0; i < n; ++i) p[i] = clean(i);
  plant(p);
  report(name, n, p);
}

// kvz_hip_inter_residual_frames_ts / kvz_hip_intra_recon_frames_ts
static void ts_case(const char *name, int n, bool lists, bool skip, const std::function<void(kvz_hip_chain_picture_ts *)> &plant)
{
  kvz_hip_chain_picture_ts r[MAX];
  for (int i = 0; i < n; ++i) r[i] = clean_ts(i, lists, skip);
  plant(r);
  report(name, n, r);
}

// ---- the named checks of the options, and the record of a single-picture entry ----
static void option(const std::string &name, bool ok) { printf("option %s: %s\n", name.c_str(), ok ? "accepted" : "refused"); }
template <typename T> static T *plus(T *p, int bytes) { return (T *)((uintptr_t)p + (unsigned)bytes); }

// the fields of a record as the loose arguments of an entry, packed again
static bool packs_to_itself(const kvz_hip_chain_picture &c)
{
  kvz_hip_chain_picture p;
  memset(&p, 0xa5, sizeof p);
  if (!chain_picture_pack(&p, &c.src, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.cus, c.intra_modes, c.coeff_y, c.coeff_u, c.coeff_v, c.cbf_out,
                          c.costs, c.lcu_qp, &c.params))
    return false;
  return p.src.y == c.src.y && p.src.u == c.src.u && p.src.v == c.src.v && p.src.stride_y == c.src.stride_y && p.src.stride_c == c.src.stride_c &&
         p.src.width == c.src.width && p.src.height == c.src.height && p.rec_y == c.rec_y && p.rec_u == c.rec_u && p.rec_v == c.rec_v &&
         p.stride_y == c.stride_y && p.stride_c == c.stride_c && p.cus == c.cus && p.intra_modes == c.intra_modes && p.coeff_y == c.coeff_y &&
         p.coeff_u == c.coeff_u && p.coeff_v == c.coeff_v && p.cbf_out == c.cbf_out && p.costs == c.costs && p.lcu_qp == c.lcu_qp &&
         p.params.qp == c.params.qp && p.params.slice_is_intra == c.params.slice_is_intra && p.params.signhide == c.params.signhide &&
         p.params.scaling_list == c.params.scaling_list && p.params.chroma == c.params.chroma;
}

static void option_cases()
{
  static kvz_hip_trskip negative_cost = { -1, 0, nullptr }, negative_with_array = { -1, 0, fake<int32_t>(9, 0) },
                        misaligned_array = { 5, 0, plus(fake<int32_t>(9, 0), 2) };
  const int32_t *q = fake<int32_t>(0, 13), *d = fake<int32_t>(0, 14);
  uint8_t *out = fake<uint8_t>(0, 15);
  option("tables both", chain_tables_ok({ q, d }));
  option("tables without quant", chain_tables_ok({ nullptr, d }));
  option("tables without dequant", chain_tables_ok({ q, nullptr }));
  option("tables quant + 4", chain_tables_ok({ plus(q, 4), d }));
  option("tables quant + 8", chain_tables_ok({ plus(q, 8), d }));
  option("tables dequant + 4", chain_tables_ok({ q, plus(d, 4) }));
  option("tables dequant + 8", chain_tables_ok({ q, plus(d, 8) }));
  option("ts with tr_skip_out", chain_trskip_ok(&skip_by_cost, out));
  option("ts without tr_skip_out", chain_trskip_ok(&skip_by_cost, nullptr));
  option("ts bit_cost -1", chain_trskip_ok(&negative_cost, out));
  option("ts bit_cost -1 with lcu_bit_cost", chain_trskip_ok(&negative_with_array, out));
  option("ts lcu_bit_cost + 2", chain_trskip_ok(&misaligned_array, out));
  for (int qp = -64; qp <= 127; ++qp) {
    kvz_hip_chain_picture p = clean(0);
    p.params.qp = qp;
    option("one qp " + std::to_string(qp), chain_one_qp_ok(p));
    p.lcu_qp = fake<int8_t>(0, 16);
    option("lcu_qp beside qp " + std::to_string(qp), chain_one_qp_ok(p));
  }
  for (int i = 0; i < 2; ++i) {
    kvz_hip_chain_picture c = clean(i);
    if (i) { c.lcu_qp = fake<int8_t>(i, 16); c.params.slice_is_intra = 1; c.params.signhide = 1; c.params.scaling_list = 1; }
    option("record " + std::to_string(i) + " packed from its fields", packs_to_itself(c));
  }
  const kvz_hip_chain_picture c = clean(0);
  kvz_hip_chain_picture p;
  option("pack without src", chain_picture_pack(&p, nullptr, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.cus, c.intra_modes, c.coeff_y, c.coeff_u,
                                                c.coeff_v, c.cbf_out, c.costs, c.lcu_qp, &c.params));
  option("pack without params", chain_picture_pack(&p, &c.src, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.cus, c.intra_modes, c.coeff_y, c.coeff_u,
                                                   c.coeff_v, c.cbf_out, c.costs, c.lcu_qp, nullptr));
}

static kvz_hip_tile_grid grid_of(int cols, int rows, int lcus_x, int lcus_y)
{
  kvz_hip_tile_grid g;
  memset(&g, 0, sizeof g);
  g.cols = cols; g.rows = rows;
  for (int i = 0; i <= cols; ++i) g.col_bd[i] = i * lcus_x / cols;
  for (int i = 0; i <= rows; ++i) g.row_bd[i] = i * lcus_y / rows;
  return g;
}

// the pool of boundaries as tests/test_gpu_chain_multi_ts.py fills it: pictures of 16 x 8 LCUs, n_grids grids of 16 x 8 tiles (26
// boundaries each), one more grid, then a 1 x 1 grid or none, then a record without a grid whose coeff_y is null
static void pool_case(const char *name, int n_grids, int last_cols, int last_rows, bool tail_grid)
{
  static kvz_hip_tile_grid full, last, one;
  full = grid_of(16, 8, 16, 8); last = grid_of(last_cols, last_rows, 16, 8); one = grid_of(1, 1, 16, 8);
  kvz_hip_chain_picture_ts r[MAX];
  const int n = n_grids + 3;
  for (int i = 0; i < n; ++i) {
    r[i] = clean_ts(i, false, true);
    r[i].pic.src.width = 1024; r[i].pic.src.height = 512;
    r[i].pic.src.stride_y = r[i].pic.stride_y = 1024;
    r[i].pic.src.stride_c = r[i].pic.stride_c = 512;
    r[i].grid = i < n_grids ? &full : i == n_grids ? &last : (i == n_grids + 1 && tail_grid) ? &one : nullptr;
  }
  r[n - 1].pic.coeff_y = nullptr;
  report(name, n, r);
}

int main()
{
  typedef kvz_hip_chain_picture P;
  typedef kvz_hip_chain_picture_ts R;
  static kvz_hip_trskip negative_cost = { -1, 0, nullptr }, negative_with_array = { -1, 0, fake<int32_t>(9, 0) },
                        misaligned_array = { 5, 0, (const int32_t *)((uintptr_t)fake<int32_t>(9, 0) + 2) };
  static kvz_hip_tile_grid one_tile = grid_of(1, 1, 1, 1), short_grid = grid_of(1, 1, 1, 1);
  short_grid.col_bd[1] = 2;                                  // the last boundary is not the picture's one LCU column

  // ---- kvz_hip_*_frames ----
  plain_case("clean", 3, [](P *) {});
  // what tests/test_gpu_chain_multi.py plants in record 2
  plain_case("coeff_y null", 3, [](P *p) { p[2].coeff_y = nullptr; });
  plain_case("width - 4", 3, [](P *p) { p[2].src.width -= 4; });
  plain_case("scaling_list set", 3, [](P *p) { p[2].params.scaling_list = 1; });
  plain_case("rec_y of record 0", 3, [](P *p) { p[2].rec_y = p[0].rec_y; });
  // the other shared outputs, and what is no output
  plain_case("cus of record 1", 3, [](P *p) { p[2].cus = p[1].cus; });
  plain_case("coeff_y of record 0", 3, [](P *p) { p[1].coeff_y = p[0].coeff_y; });
  plain_case("shared source and chroma", 3, [](P *p) { p[2].src = p[0].src; p[2].rec_u = p[0].rec_u; p[2].coeff_v = p[0].coeff_v; });
  plain_case("negative qp", 3, [](P *p) { p[1].params.qp = -1; });
  plain_case("negative qp with lcu_qp", 3, [](P *p) { p[1].params.qp = -1; p[1].lcu_qp = fake<int8_t>(1, 16); });
  plain_case("qp 60", 3, [](P *p) { p[1].params.qp = 60; });
  plain_case("intra_modes null", 3, [](P *p) { p[1].intra_modes = nullptr; });
  plain_case("costs misaligned", 3, [](P *p) { p[0].costs = (kvz_hip_inter_residual_cost *)((uintptr_t)p[0].costs + 2); });
  plain_case("coeff_u misaligned", 3, [](P *p) { p[2].coeff_u = (kvz_hip_coeff *)((uintptr_t)p[2].coeff_u + 8); });
  plain_case("coeff_u misaligned in 4:0:0", 3, [](P *p) { p[2].coeff_u = (kvz_hip_coeff *)((uintptr_t)p[2].coeff_u + 8); p[2].params.chroma = 0; });
  plain_case("4:0:0 without chroma planes", 3, [](P *p) { p[0].params.chroma = 0; p[0].rec_u = p[0].rec_v = nullptr; p[0].coeff_u = p[0].coeff_v = nullptr; p[0].src.u = p[0].src.v = nullptr; });
  plain_case("optional outputs null", 3, [](P *p) { p[1].cbf_out = nullptr; p[1].costs = nullptr; });
  plain_case("stride_c short", 3, [](P *p) { p[0].stride_c = 31; });
  plain_case("height 16392", 3, [](P *p) { p[2].src.height = 16392; });
  plain_case("records 1 and 2", 3, [](P *p) { p[1].cus = nullptr; p[2].rec_y = nullptr; });

  // ---- kvz_hip_*_frames_ts ----
  ts_case("clean skip", 3, false, true, [](R *) {});
  ts_case("clean lists", 3, true, false, [](R *) {});
  ts_case("clean lists and skip", 3, true, true, [](R *) {});
  // what tests/test_gpu_chain_multi_ts.py plants, at the indices it plants them
  ts_case("tables among none", 3, false, true, [](R *r) { r[2].tables = clean_ts(2, true, false).tables; r[2].pic.params.scaling_list = 1; });
  ts_case("no tables among tables", 3, true, false, [](R *r) { r[1].tables.quant = r[1].tables.dequant = nullptr; r[1].pic.params.scaling_list = 0; });
  ts_case("ts among none", 3, true, false, [](R *r) { r[2].ts = &skip_by_cost; r[2].tr_skip_out = fake<uint8_t>(2, 15); });
  ts_case("no ts among ts", 3, true, true, [](R *r) { r[1].ts = nullptr; });
  ts_case("scaling_list without tables", 3, false, true, [](R *r) { r[1].pic.params.scaling_list = 1; });
  ts_case("tables without scaling_list", 3, true, false, [](R *r) { r[1].pic.params.scaling_list = 0; });
  ts_case("a null table", 3, true, false, [](R *r) { r[2].tables.dequant = nullptr; });
  ts_case("ts without tr_skip_out", 3, false, true, [](R *r) { r[1].tr_skip_out = nullptr; });
  ts_case("tr_skip_out of record 1", 4, true, true, [](R *r) { r[3].tr_skip_out = r[1].tr_skip_out; });      // that test's index: a fourth record
  ts_case("short grid", 3, true, true, [](R *r) { r[0].grid = &short_grid; });
  pool_case("pool 256 then a null coeff_y", 9, 12, 8, false);
  pool_case("pool 257", 9, 9, 8, true);
  // homogeneity is measured on record 0
  ts_case("record 0 alone with tables", 3, false, true, [](R *r) { r[0].tables = clean_ts(0, true, false).tables; r[0].pic.params.scaling_list = 1; });
  // shared outputs
  ts_case("ts rec_y of record 0", 3, false, true, [](R *r) { r[2].pic.rec_y = r[0].pic.rec_y; });
  ts_case("ts cus of record 0", 3, true, false, [](R *r) { r[1].pic.cus = r[0].pic.cus; });
  ts_case("ts coeff_y of record 1", 3, true, true, [](R *r) { r[2].pic.coeff_y = r[1].pic.coeff_y; });
  ts_case("tr_skip_out of record 0", 3, false, true, [](R *r) { r[2].tr_skip_out = r[0].tr_skip_out; });
  ts_case("tr_skip_out equal without ts", 3, true, false, [](R *r) { r[2].tr_skip_out = r[0].tr_skip_out = fake<uint8_t>(0, 15); });
  ts_case("shared tables", 3, true, false, [](R *r) { r[2].tables = r[0].tables; });
  // the rest of a record's own checks
  ts_case("a misaligned table", 3, true, true, [](R *r) { r[1].tables.quant += 1; });
  ts_case("negative bit_cost", 3, false, true, [](R *r) { r[1].ts = &negative_cost; });
  ts_case("negative bit_cost with lcu_bit_cost", 3, false, true, [](R *r) { r[1].ts = &negative_with_array; });
  ts_case("misaligned lcu_bit_cost", 3, false, true, [](R *r) { r[2].ts = &misaligned_array; });
  ts_case("ts negative qp", 3, true, false, [](R *r) { r[2].pic.params.qp = -3; });
  ts_case("ts negative qp with lcu_qp", 3, true, false, [](R *r) { r[2].pic.params.qp = -3; r[2].pic.lcu_qp = fake<int8_t>(2, 16); });
  ts_case("ts intra_modes null", 3, false, true, [](R *r) { r[0].pic.intra_modes = nullptr; });
  ts_case("grid of one tile", 3, false, true, [](R *r) { r[1].grid = &one_tile; });
  // two defects in one record: the first check in the entries' order names the reason
  ts_case("homogeneity before a null table", 3, false, true, [](R *r) { r[1].tables.quant = fake<int32_t>(1, 13); });
  ts_case("table before arguments", 3, true, true, [](R *r) { r[1].tables.dequant = nullptr; r[1].pic.rec_y = nullptr; });
  ts_case("arguments before ts", 3, false, true, [](R *r) { r[2].pic.params.scaling_list = 1; r[2].tr_skip_out = nullptr; });
  ts_case("ts before qp", 3, false, true, [](R *r) { r[1].tr_skip_out = nullptr; r[1].pic.params.qp = -1; });
  ts_case("qp before grid", 3, true, true, [](R *r) { r[1].pic.params.qp = -1; r[1].grid = &short_grid; });
  ts_case("qp before shared", 3, true, false, [](R *r) { r[2].pic.params.qp = -1; r[2].pic.rec_y = r[0].pic.rec_y; });
  ts_case("grid before shared", 3, false, true, [](R *r) { r[2].grid = &short_grid; r[2].pic.rec_y = r[0].pic.rec_y; });
  ts_case("record 1 before record 2", 3, true, true, [](R *r) { r[1].pic.cus = r[0].pic.cus; r[2].ts = nullptr; });
  option_cases();
  return 0;
}
"""


def both(v):
    return (v, v)


# case -> (inter entry, intra entry): None where the call is accepted, else (index of the first refused record, reason)
EXPECTED = {
    "clean": both(None),
    "coeff_y null": both((2, PLAIN)),
    "width - 4": both((2, PLAIN)),
    "scaling_list set": both((2, PLAIN)),
    "rec_y of record 0": both((2, PLAIN)),
    "cus of record 1": both((2, PLAIN)),
    "coeff_y of record 0": both((1, PLAIN)),
    "shared source and chroma": both(None),
    "negative qp": both((1, PLAIN)),
    "negative qp with lcu_qp": both(None),
    "qp 60": both(None),                                     # the one-QP entries set no upper bound
    "intra_modes null": (None, (1, PLAIN)),
    "costs misaligned": both((0, PLAIN)),
    "coeff_u misaligned": both((2, PLAIN)),
    "coeff_u misaligned in 4:0:0": both(None),
    "4:0:0 without chroma planes": both(None),
    "optional outputs null": both(None),
    "stride_c short": both((0, PLAIN)),
    "height 16392": both((2, PLAIN)),
    "records 1 and 2": both((1, PLAIN)),
    "clean skip": both(None),
    "clean lists": both(None),
    "clean lists and skip": both(None),
    "tables among none": both((2, HOMOGENEOUS)),
    "no tables among tables": both((1, HOMOGENEOUS)),
    "ts among none": both((2, HOMOGENEOUS)),
    "no ts among ts": both((1, HOMOGENEOUS)),
    "scaling_list without tables": both((1, ARGS)),
    "tables without scaling_list": both((1, ARGS)),
    "a null table": both((2, TABLE)),
    "ts without tr_skip_out": both((1, TS)),
    "tr_skip_out of record 1": both((3, SHARED)),
    "short grid": (None, (0, GRID)),                          # the inter stage does not depend on tiles and does not read the grid
    "pool 256 then a null coeff_y": both((11, ARGS)),
    "pool 257": ((11, ARGS), (10, POOL)),
    "record 0 alone with tables": both((1, HOMOGENEOUS)),
    "ts rec_y of record 0": both((2, SHARED)),
    "ts cus of record 0": both((1, SHARED)),
    "ts coeff_y of record 1": both((2, SHARED)),
    "tr_skip_out of record 0": both((2, SHARED)),
    "tr_skip_out equal without ts": both(None),
    "shared tables": both(None),
    "a misaligned table": both((1, TABLE)),
    "negative bit_cost": both((1, TS)),
    "negative bit_cost with lcu_bit_cost": both(None),
    "misaligned lcu_bit_cost": both((2, TS)),
    "ts negative qp": both((2, QP)),
    "ts negative qp with lcu_qp": both(None),
    "ts intra_modes null": (None, (0, ARGS)),
    "grid of one tile": both(None),
    "homogeneity before a null table": both((1, HOMOGENEOUS)),
    "table before arguments": both((1, TABLE)),
    "arguments before ts": both((2, ARGS)),
    "ts before qp": both((1, TS)),
    "qp before grid": both((1, QP)),
    "qp before shared": both((2, QP)),
    "grid before shared": ((2, SHARED), (2, GRID)),
    "record 1 before record 2": both((1, SHARED)),
}


# the named checks and the packing: True where accepted
OPTIONS = {
    "tables both": True,
    "tables without quant": False,
    "tables without dequant": False,
    "tables quant + 4": False,
    "tables quant + 8": False,
    "tables dequant + 4": False,
    "tables dequant + 8": False,
    "ts with tr_skip_out": True,
    "ts without tr_skip_out": False,
    "ts bit_cost -1": False,
    "ts bit_cost -1 with lcu_bit_cost": True,
    "ts lcu_bit_cost + 2": False,
    "record 0 packed from its fields": True,
    "record 1 packed from its fields": True,
    "pack without src": False,
    "pack without params": False,
}
# what make_consts decided for the probe of the one-QP rule (the module's docstring): refused below 0, accepted from 0
OPTIONS.update({"one qp %d" % qp: qp >= 0 for qp in range(-64, 128)})
OPTIONS.update({"lcu_qp beside qp %d" % qp: True for qp in range(-64, 128)})


@functools.lru_cache(maxsize=None)
def program_output():
    """the program's lines, compiled and run once: ({case: {stage: verdict}}, {option: accepted})"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "chain_host_checks.cpp"), os.path.join(tmp, "chain_host_checks")
        with open(src, "w") as f:
            f.write(PROGRAM)
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
               "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"), src, "-o", exe]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    got, options = {}, {}
    for line in r.stdout.splitlines():
        case, _, verdict = line.partition(": ")
        if case.startswith("option "):
            assert verdict in ("accepted", "refused"), line
            options[case[len("option "):]] = verdict == "accepted"
            continue
        name, _, stage = case.rpartition("/")
        index, _, reason = verdict.partition(" ")
        got.setdefault(name, {})[stage] = None if verdict == "ok" else (int(index), reason)
    return got, options


def test_record_checks_report_the_first_refused_record_and_its_reason():
    got, _ = program_output()
    assert sorted(got) == sorted(EXPECTED)
    for name, (inter, intra) in EXPECTED.items():
        assert got[name] == {"inter": inter, "intra": intra}, name


def test_option_checks_and_the_record_of_a_single_picture_entry():
    _, options = program_output()
    assert sorted(options) == sorted(OPTIONS)
    for name, accepted in OPTIONS.items():
        assert options[name] == accepted, name

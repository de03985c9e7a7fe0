"""CPU: the record checks of the filter and prediction stages (kvazaar_amd/csrc/chain_host.h) without a device.

kvz_hip_cu_qp_frames, kvz_hip_deblock_frames, kvz_hip_sao_stats_frames, kvz_hip_sao_frames and kvz_hip_inter_recon_frames return
KVZ_HIP_ERR_NO_DEVICE before they look at a record, so on a machine without a GPU nothing ever ran their checks.  As
tests/test_chain_host_checks.py does for the residual stages, a stand-alone C++ program includes the header with kvz_hip.h alone, builds
records on fake, suitably aligned pointer values (the checks compare pointers and never follow them; only a kvz_hip_tile_grid and the
pool of reference pictures are read, and those are host memory), hands them to the one function that each entry calls on its records
(filter_records_why, recon_records_why: the record's own checks, its grid into the pool of boundaries, the outputs of the earlier
records) and prints, per case and stage, the index of the first refused record and its reason.  It is compiled with the address and undefined-behaviour sanitizers, linked statically, and run as a child.

A case plants its defect in one table of records that all four filter stages then read, so a case names what each stage says.  The
records are 64x64 and 8x8 in turn, record 2 is the ragged 200x136 picture of tests/test_gpu_chain_filter_multi.py; the pool of
boundaries overflows on 1024x512 pictures with 16x8 tiles.  The expected indices of the defects that
tests/test_gpu_chain_filter_multi.py and tests/test_gpu_inter_recon_multi.py plant are the ones those tests assert; the expected
reasons are the message strings of the entries as they stood before the checks moved into the header, copied here as literals.  The
order of an entry's checks is pinned by one case per adjacent pair of them.

The same program runs the predicates that a single-picture entry composes where they differ from the record check -- deblocking
without an upper bound on the size, motion compensation without aligned planes -- and the packing of a single-picture entry's loose
arguments into a record."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reasons, as the five entries spelled them
CHROMA = "deblock.chroma differs from chroma"
GRID = "invalid tile grid"
POOL = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record"
SHARED = "an output shared with another picture"
PLANES = "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8"
QP_PTR = "a null pointer or a misaligned cus"
QP_SIZE = "width / height must be multiples of 8 in 8..16384"
QP_CHAIN = "start_qp outside 0..51 or chain_rows other than 0 and 1"
DEBLOCK = "planes and the SCU map must be 4-byte aligned, width / height multiples of 8 in 8..16384, strides >= the width"
SRC = "src.width / src.height differ from width / height"
STATS_OUT = "stats is null, or stats or cands misaligned"
CHROMA_PLANE = "a chroma plane is null or misaligned, or its stride is"
SAO_LUMA = "sao_luma is null or misaligned, or dst_y is rec_y"
SAO_CHROMA = "sao_chroma or a chroma plane is null or misaligned, a chroma stride is, or a dst plane is its rec plane"
R_PTR = "pred_y or cus is null, or cus misaligned"
R_SIZE = "width / height must be multiples of 8, stride_y >= the width"
R_NREFS = "n_refs outside 1..16"
R_CHROMA = "a chroma plane is null, or stride_c below half the width"
R_INDEX = "a reference index outside the pool"
R_REF = "a named pool picture of another size, with a missing plane or a short stride"
R_SHARED = "pred_y shared with another picture"
R_GRID = "the pictures of the call exceed the grid"
R_DST = "a destination plane is a named pool plane"

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
template <typename T> static T *plus(T *p, int bytes) { return (T *)((uintptr_t)p + (unsigned)bytes); }
enum { MAX = KVZ_HIP_MAX_CHAIN_PICTURES };
typedef kvz_hip_filter_picture P;
typedef kvz_hip_recon_picture R;
typedef kvz_hip_ref_picture Q;

static void resize(P &p, int w, int h)
{
  p.width = p.src.width = w; p.height = p.src.height = h;
  p.stride_y = p.dst_stride_y = p.src.stride_y = (uint32_t)w;
  p.stride_c = p.dst_stride_c = p.src.stride_c = (uint32_t)w / 2;
}
// record i of a clean call: 64x64 and 8x8 in turn, record 2 ragged; 4:2:0, cands given, no grid
static P clean(int i)
{
  P p;
  memset(&p, 0, sizeof p);
  resize(p, i == 2 ? 200 : i % 2 ? 8 : 64, i == 2 ? 136 : i % 2 ? 8 : 64);
  p.chroma = p.deblock.chroma = 1;
  p.src.y = fake<kvz_hip_pixel>(i, 0); p.src.u = fake<kvz_hip_pixel>(i, 1); p.src.v = fake<kvz_hip_pixel>(i, 2);
  p.rec_y = fake<kvz_hip_pixel>(i, 3); p.rec_u = fake<kvz_hip_pixel>(i, 4); p.rec_v = fake<kvz_hip_pixel>(i, 5);
  p.dst_y = fake<kvz_hip_pixel>(i, 6); p.dst_u = fake<kvz_hip_pixel>(i, 7); p.dst_v = fake<kvz_hip_pixel>(i, 8);
  p.cus = fake<kvz_hip_cu_info>(i, 9); p.cbf = fake<uint8_t>(i, 10); p.lcu_qp = fake<int8_t>(i, 11); p.lcu_last_qp = fake<int8_t>(i, 12);
  p.stats = fake<kvz_hip_sao_lcu_stats>(i, 13); p.cands = fake<kvz_hip_sao_lcu_cand>(i, 14);
  p.sao_luma = fake<kvz_hip_sao_info>(i, 15); p.sao_chroma = fake<kvz_hip_sao_info>(i, 16);
  p.deblock.qp = 30; p.cu_qp.start_qp = 30;
  return p;
}

static void report(const char *name, const char *stage, int at, const char *why)
{
  if (!why) { printf("%s/%s: ok\n", name, stage); return; }
  // through refuse_picture, as the entries do: the message names the record
  refuse_picture("entry", at, why);
  char head[64];
  snprintf(head, sizeof head, "entry: invalid argument in picture %d (", at);
  if (last_message != std::string(head) + why + ")") printf("%s/%s: MESSAGE %s\n", name, stage, last_message.c_str());
  else printf("%s/%s: %d %s\n", name, stage, at, why);
}

// the four entries' one call on n records, with the arguments that each entry gives: the statistics take no tiles
static void filter_records(const char *name, int n, const P *r)
{
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  pic_tiles tiles[MAX];
  int used = 0, none = 0, at = 0;
  const char *why = filter_records_why(r, n, cu_qp_record_why, cu_qp_output_shared, bounds, used, tiles, &at);
  report(name, "qp", at, why);
  why = filter_records_why(r, n, deblock_record_why, deblock_output_shared, bounds, used = 0, tiles, &at);
  report(name, "deblock", at, why);
  why = filter_records_why(r, n, sao_stats_record_why, sao_stats_output_shared, nullptr, none, nullptr, &at);
  report(name, "stats", at, why);
  why = filter_records_why(r, n, sao_record_why, sao_output_shared, bounds, used = 0, tiles, &at);
  report(name, "sao", at, why);
}
static void filter_case(const char *name, int n, const std::function<void(P *)> &plant)
{
  P p[MAX];
  for (int i = 0; i < n; ++i) p[i] = clean(i);
  plant(p);
  filter_records(name, n, p);
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

// the pool of boundaries: pictures of 16 x 8 LCUs, n_grids grids of 16 x 8 tiles (26 boundaries each), then `last`, then a record
// without a grid that `plant` may change
static void pool_case(const char *name, int n_grids, const kvz_hip_tile_grid *last, const std::function<void(P *, int)> &plant)
{
  static kvz_hip_tile_grid full;
  full = grid_of(16, 8, 16, 8);
  P p[MAX];
  const int n = n_grids + 2;
  for (int i = 0; i < n; ++i) {
    p[i] = clean(i);
    resize(p[i], 1024, 512);
    p[i].grid = i < n_grids ? &full : i == n_grids ? last : nullptr;
  }
  plant(p, n - 1);
  filter_records(name, n, p);
}

// ---- motion compensation: the pictures of tests/test_gpu_inter_recon_multi.py.  Pictures 0 and 1 are 64x64, 4:2:0, over pool pictures
// (0, 1) and (2, 3); picture 2 is 72x40, 4:0:0, over pool picture 4 twice, with 2 of its 16 table entries in use ----
static Q pool_picture(int k, int w, int h)
{
  return Q{ fake<kvz_hip_pixel>(20 + k, 0), fake<kvz_hip_pixel>(20 + k, 1), fake<kvz_hip_pixel>(20 + k, 2), (uint32_t)w, (uint32_t)w / 2, w, h };
}
static R recon_picture(int i, int w, int h, int chroma, int r0, int r1)
{
  R p;
  memset(&p, 0, sizeof p);
  p.pred_y = fake<kvz_hip_pixel>(i, 0); p.pred_u = fake<kvz_hip_pixel>(i, 1); p.pred_v = fake<kvz_hip_pixel>(i, 2);
  p.stride_y = (uint32_t)w; p.stride_c = (uint32_t)w / 2; p.width = w; p.height = h;
  p.cus = fake<kvz_hip_cu_info>(i, 3);
  p.refs[0] = (uint8_t)r0; p.refs[1] = (uint8_t)r1;
  p.params.chroma = chroma; p.params.n_refs = 2;
  return p;
}
static void recon_case(const char *name, const std::function<void(R *, Q *, int &)> &plant)
{
  R p[MAX] = { recon_picture(0, 64, 64, 1, 0, 1), recon_picture(1, 64, 64, 1, 2, 3), recon_picture(2, 72, 40, 0, 4, 4) };
  Q pool[KVZ_HIP_RECON_POOL_PICTURES];
  memset(pool, 0x5a, sizeof pool);                             // what no record names is garbage
  for (int k = 0; k < 5; ++k) pool[k] = k < 4 ? pool_picture(k, 64, 64) : pool_picture(k, 72, 40);
  int n_pool = 5;
  plant(p, pool, n_pool);
  // the entry's one call: every record, then the pass over the destinations
  bool named[KVZ_HIP_RECON_POOL_PICTURES] = { false };
  unsigned long long groups = 0;
  int first_wg[MAX], at = 0;
  report(name, "recon", at, recon_records_why(p, 3, pool, n_pool, named, first_wg, groups, &at));
}

// ---- the predicates where a single-picture entry differs from the record check, and the records of the single-picture entries ----
static void option(const std::string &name, bool ok) { printf("option %s: %s\n", name.c_str(), ok ? "accepted" : "refused"); }
static bool same(const P &a, const P &b) { return memcmp(&a, &b, sizeof a) == 0; }

static void option_cases()
{
  // deblocking: the single entries set no upper bound on the size, the record check does
  P wide = clean(0);
  resize(wide, 16392, 64);
  option("deblock single 16392", deblock_luma_ok(wide) && deblock_chroma_ok(wide));
  option("deblock record 16392", deblock_record_why(wide) == nullptr);
  option("cu_qp size 16392", picture_ok(16392, 64));
  option("sao luma planes 16392", sao_luma_planes_ok(wide));
  // motion compensation asks for no aligned plane, SAO does
  R odd = recon_picture(0, 64, 64, 1, 0, 1);
  odd.pred_y = plus(odd.pred_y, 1); odd.pred_u = plus(odd.pred_u, 3); odd.stride_y = 65; odd.stride_c = 33;
  option("recon odd planes", recon_arrays_ok(odd) && recon_luma_ok(odd) && recon_chroma_ok(odd));
  Q odd_ref = pool_picture(0, 64, 64);
  odd_ref.y = plus(odd_ref.y, 1); odd_ref.stride_y = 67;
  option("recon odd reference", ref_ok(odd_ref, 1, 64, 64) && refs_ok(&odd_ref, 1, 1, 64, 64));
  P odd_sao = clean(0);
  odd_sao.rec_y = plus(odd_sao.rec_y, 1);
  option("sao odd rec_y", sao_luma_planes_ok(odd_sao));
  option("recon size 16392", recon_luma_ok(recon_picture(0, 16392, 64, 0, 0, 0)));

  // the fields of a record as the loose arguments of an entry, packed again: what the stage does not take is zero
  static kvz_hip_tile_grid grid = grid_of(2, 2, 4, 3);
  for (int i = 0; i < 3; ++i) {
    const std::string rec = "record " + std::to_string(i);
    P c = clean(i), p, e;
    c.grid = i == 2 ? &grid : nullptr; c.cu_qp.chain_rows = i % 2; c.deblock.slice_is_b = i; c.deblock.ref_LX[1][3] = 7;
    memset(&e, 0, sizeof e);
    e.width = c.width; e.height = c.height; e.cus = c.cus; e.cbf = c.cbf; e.lcu_qp = c.lcu_qp; e.lcu_last_qp = c.lcu_last_qp; e.grid = c.grid; e.cu_qp = c.cu_qp;
    memset(&p, 0xa5, sizeof p);
    option(rec + " packed by cu_qp", cu_qp_pack(&p, c.cus, c.cbf, c.width, c.height, c.lcu_qp, c.lcu_last_qp, c.grid, &c.cu_qp) && same(p, e));
    memset(&e, 0, sizeof e);
    e.width = c.width; e.height = c.height; e.chroma = c.deblock.chroma; e.rec_y = c.rec_y; e.rec_u = c.rec_u; e.rec_v = c.rec_v;
    e.stride_y = c.stride_y; e.stride_c = c.stride_c; e.cus = c.cus; e.grid = c.grid; e.deblock = c.deblock;
    memset(&p, 0xa5, sizeof p);
    option(rec + " packed by deblock", deblock_pack(&p, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.width, c.height, c.cus, c.grid, &c.deblock) && same(p, e));
    memset(&e, 0, sizeof e);
    e.width = c.width; e.height = c.height; e.chroma = c.chroma; e.src = c.src; e.rec_y = c.rec_y; e.rec_u = c.rec_u; e.rec_v = c.rec_v;
    e.stride_y = c.stride_y; e.stride_c = c.stride_c; e.stats = c.stats; e.cands = c.cands;
    memset(&p, 0xa5, sizeof p);
    option(rec + " packed by sao_stats", sao_stats_pack(&p, &c.src, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.chroma, c.stats, c.cands) && same(p, e));
    memset(&e, 0, sizeof e);
    e.width = c.width; e.height = c.height; e.chroma = c.chroma; e.rec_y = c.rec_y; e.rec_u = c.rec_u; e.rec_v = c.rec_v; e.stride_y = c.stride_y;
    e.stride_c = c.stride_c; e.dst_y = c.dst_y; e.dst_u = c.dst_u; e.dst_v = c.dst_v; e.dst_stride_y = c.dst_stride_y; e.dst_stride_c = c.dst_stride_c;
    e.sao_luma = c.sao_luma; e.sao_chroma = c.sao_chroma; e.grid = c.grid;
    memset(&p, 0xa5, sizeof p);
    sao_pack(&p, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.dst_y, c.dst_stride_y, c.dst_u, c.dst_v, c.dst_stride_c, c.width, c.height, c.sao_luma,
             c.sao_chroma, c.chroma, c.grid);
    option(rec + " packed by sao", same(p, e));
    // motion compensation: the table of the single entry is the pool, reference k is pool picture k
    R rc = recon_picture(i, c.width, c.height, i != 2, 0, 1), rp;
    for (int k = 0; k < 16; ++k) rc.refs[k] = (uint8_t)k;
    rc.params.ref_LX[1][2] = 9;
    memset(&rp, 0xa5, sizeof rp);
    option(rec + " packed by inter_recon", recon_pack(&rp, rc.pred_y, rc.stride_y, rc.pred_u, rc.pred_v, rc.stride_c, rc.width, rc.height, rc.cus, fake<Q>(0, 0),
                                                      &rc.params) && memcmp(&rp, &rc, sizeof rc) == 0);
  }
  const P c = clean(0);
  P p;
  option("cu_qp pack without params", cu_qp_pack(&p, c.cus, c.cbf, c.width, c.height, c.lcu_qp, c.lcu_last_qp, nullptr, nullptr));
  option("deblock pack without params", deblock_pack(&p, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.width, c.height, c.cus, nullptr, nullptr));
  option("sao_stats pack without src", sao_stats_pack(&p, nullptr, c.rec_y, c.stride_y, c.rec_u, c.rec_v, c.stride_c, c.chroma, c.stats, c.cands));
  const R rc = recon_picture(0, 64, 64, 1, 0, 1);
  R rp;
  option("inter_recon pack without refs", recon_pack(&rp, rc.pred_y, rc.stride_y, rc.pred_u, rc.pred_v, rc.stride_c, 64, 64, rc.cus, nullptr, &rc.params));
  option("inter_recon pack without params", recon_pack(&rp, rc.pred_y, rc.stride_y, rc.pred_u, rc.pred_v, rc.stride_c, 64, 64, rc.cus, fake<Q>(0, 0), nullptr));
}

int main()
{
  // ---- the four filter entries ----
  filter_case("clean", 3, [](P *) {});
  filter_case("clean sixteen", 16, [](P *) {});
  // what tests/test_gpu_chain_filter_multi.py plants in the last record, the ragged one
  filter_case("deblock.chroma 0", 3, [](P *p) { p[2].deblock.chroma = 0; });
  filter_case("width - 4", 3, [](P *p) { p[2].width -= 4; });
  filter_case("height 4", 3, [](P *p) { p[2].height = 4; });
  filter_case("cus null", 3, [](P *p) { p[2].cus = nullptr; });
  filter_case("cbf null", 3, [](P *p) { p[2].cbf = nullptr; });
  filter_case("lcu_qp null", 3, [](P *p) { p[2].lcu_qp = nullptr; });
  filter_case("lcu_last_qp null", 3, [](P *p) { p[2].lcu_last_qp = nullptr; });
  filter_case("rec_y null", 3, [](P *p) { p[2].rec_y = nullptr; });
  filter_case("rec_u null", 3, [](P *p) { p[2].rec_u = nullptr; });
  filter_case("stats null", 3, [](P *p) { p[2].stats = nullptr; });
  filter_case("src.y null", 3, [](P *p) { p[2].src.y = nullptr; });
  filter_case("src.v null", 3, [](P *p) { p[2].src.v = nullptr; });
  filter_case("sao_luma null", 3, [](P *p) { p[2].sao_luma = nullptr; });
  filter_case("sao_chroma null", 3, [](P *p) { p[2].sao_chroma = nullptr; });
  filter_case("dst_y null", 3, [](P *p) { p[2].dst_y = nullptr; });
  filter_case("dst_v null", 3, [](P *p) { p[2].dst_v = nullptr; });
  filter_case("cus + 2", 3, [](P *p) { p[2].cus = plus(p[2].cus, 2); });
  filter_case("rec_y + 1", 3, [](P *p) { p[2].rec_y = plus(p[2].rec_y, 1); });
  filter_case("stats + 2", 3, [](P *p) { p[2].stats = plus(p[2].stats, 2); });
  filter_case("cands + 1", 3, [](P *p) { p[2].cands = plus(p[2].cands, 1); });
  filter_case("src.width + 8", 3, [](P *p) { p[2].src.width += 8; });
  filter_case("sao_luma + 2", 3, [](P *p) { p[2].sao_luma = plus(p[2].sao_luma, 2); });
  filter_case("stride_y - 4", 3, [](P *p) { p[2].stride_y -= 4; });
  filter_case("src.stride_y - 4", 3, [](P *p) { p[2].src.stride_y -= 4; });
  filter_case("dst_stride_y - 4", 3, [](P *p) { p[2].dst_stride_y -= 4; });
  filter_case("stride_c - 4", 3, [](P *p) { p[2].stride_c -= 4; });
  filter_case("dst_y is rec_y", 3, [](P *p) { p[2].dst_y = p[2].rec_y; });
  filter_case("dst_u is rec_u", 3, [](P *p) { p[2].dst_u = p[2].rec_u; });
  filter_case("cus of record 0", 3, [](P *p) { p[2].cus = p[0].cus; });
  filter_case("lcu_last_qp of record 1", 3, [](P *p) { p[2].lcu_last_qp = p[1].lcu_last_qp; });
  filter_case("rec_y of record 0", 3, [](P *p) { p[2].rec_y = p[0].rec_y; });
  filter_case("stats of record 1", 3, [](P *p) { p[2].stats = p[1].stats; });
  filter_case("dst_y of record 0", 3, [](P *p) { p[2].dst_y = p[0].dst_y; });
  // that test's malformed grids of the ragged picture, 4 x 3 LCUs: from col_bd 0, 1, 4 and row_bd 0, 2, 3
  static kvz_hip_tile_grid good = grid_of(2, 2, 4, 3), bad[12];
  good.col_bd[1] = 1; good.row_bd[1] = 2;
  for (int k = 0; k < 12; ++k) bad[k] = good;
  bad[0].cols = 0; bad[1].cols = 48; bad[2].rows = 0; bad[3].rows = -1; bad[4].rows = 48; bad[5].col_bd[0] = 1; bad[6].row_bd[0] = -1; bad[7].row_bd[1] = 0;
  bad[8].cols = 3; bad[8].col_bd[1] = 2; bad[8].col_bd[2] = 1; bad[8].col_bd[3] = 4;
  bad[9].col_bd[2] = 3; bad[10].row_bd[2] = 4; bad[11].col_bd[2] = 5;
  filter_case("ragged grid", 3, [](P *p) { p[2].grid = &good; });
  static char names[12][24];
  for (int k = 0; k < 12; ++k) {
    snprintf(names[k], sizeof names[k], "bad grid %d", k);
    filter_case(names[k], 3, [k](P *p) { p[2].grid = &bad[k]; });
  }
  filter_case("start_qp -1", 3, [](P *p) { p[2].cu_qp.start_qp = -1; });
  filter_case("start_qp 52", 3, [](P *p) { p[2].cu_qp.start_qp = 52; });
  filter_case("start_qp 0 and 51", 3, [](P *p) { p[0].cu_qp.start_qp = 0; p[2].cu_qp.start_qp = 51; });
  filter_case("chain_rows 2", 3, [](P *p) { p[2].cu_qp.chain_rows = 2; });
  filter_case("chain_rows -1", 3, [](P *p) { p[2].cu_qp.chain_rows = -1; });
  filter_case("chain_rows 1", 3, [](P *p) { p[2].cu_qp.chain_rows = 1; });
  filter_case("cus null in the middle", 3, [](P *p) { p[1].cus = nullptr; });
  // the pool: nine grids of 26 boundaries fit, the tenth does not; a grid of 12 x 8 tiles fills it to the last of the 256
  static kvz_hip_tile_grid full = grid_of(16, 8, 16, 8), fill = grid_of(12, 8, 16, 8), bad_wide = grid_of(16, 8, 16, 8);
  bad_wide.col_bd[16] = 17;
  pool_case("pool 260", 9, &full, [](P *, int) {});
  pool_case("pool 256", 9, &fill, [](P *, int) {});
  // ---- what is accepted ----
  filter_case("4:0:0 without chroma planes", 3, [](P *p) {
    p[1].chroma = p[1].deblock.chroma = 0;
    p[1].rec_u = p[1].rec_v = p[1].dst_u = p[1].dst_v = nullptr; p[1].src.u = p[1].src.v = nullptr; p[1].sao_chroma = nullptr; p[1].stride_c = p[1].dst_stride_c = 1;
  });
  filter_case("cands null", 3, [](P *p) { p[2].cands = nullptr; });
  filter_case("cands null in two records", 3, [](P *p) { p[0].cands = p[2].cands = nullptr; });
  filter_case("cands of record 0", 3, [](P *p) { p[2].cands = p[0].cands; });
  filter_case("shared inputs", 3, [](P *p) {
    p[2].cbf = p[0].cbf; p[2].lcu_qp = p[0].lcu_qp; p[2].src = p[0].src; resize(p[2], 64, 64); p[2].sao_luma = p[0].sao_luma; p[2].sao_chroma = p[0].sao_chroma;
    p[1].deblock = p[0].deblock;
  });
  filter_case("width 16384", 3, [](P *p) { resize(p[0], 16384, 8); });
  // ---- two defects in one record: the first check in the entry's order names the reason ----
  filter_case("width 16392", 3, [](P *p) { resize(p[1], 16392, 8); });
  filter_case("cus null, width - 4", 3, [](P *p) { p[1].cus = nullptr; p[1].width -= 4; p[1].src.width -= 4; });
  filter_case("width - 4, start_qp 52", 3, [](P *p) { p[1].width -= 4; p[1].src.width -= 4; p[1].cu_qp.start_qp = 52; });
  filter_case("start_qp 52, deblock.chroma 0", 3, [](P *p) { p[1].cu_qp.start_qp = 52; p[1].deblock.chroma = 0; });
  filter_case("deblock.chroma 0, bad grid", 3, [](P *p) { p[2].deblock.chroma = 0; p[2].grid = &bad[0]; });
  filter_case("deblock.chroma 0, src.width + 8", 3, [](P *p) { p[2].deblock.chroma = 0; p[2].src.width += 8; });
  filter_case("deblock.chroma 0, sao_luma null, rec_y + 1", 3, [](P *p) { p[2].deblock.chroma = 0; p[2].sao_luma = nullptr; p[2].rec_y = plus(p[2].rec_y, 1); });
  filter_case("src.width + 8, stats null", 3, [](P *p) { p[2].src.width += 8; p[2].stats = nullptr; });
  filter_case("stats null, sao_luma null, rec_y null", 3, [](P *p) { p[2].stats = nullptr; p[2].sao_luma = nullptr; p[2].rec_y = nullptr; });
  filter_case("rec_y + 1, rec_u null, sao_chroma null", 3, [](P *p) { p[2].rec_y = plus(p[2].rec_y, 1); p[2].rec_u = nullptr; p[2].sao_chroma = nullptr; });
  filter_case("rec_u null, bad grid, stats of record 0", 3, [](P *p) { p[2].rec_u = nullptr; p[2].grid = &bad[0]; p[2].stats = p[0].stats; });
  filter_case("bad grid, shared outputs", 3, [](P *p) { p[2].grid = &bad[0]; p[2].cus = p[0].cus; p[2].rec_y = p[0].rec_y; p[2].dst_y = p[0].dst_y; });
  pool_case("bad grid where the pool is full", 9, &bad_wide, [](P *, int) {});
  pool_case("pool 260, shared outputs", 9, &full, [](P *p, int) { p[9].cus = p[0].cus; p[9].rec_y = p[0].rec_y; p[9].dst_y = p[0].dst_y; });
  pool_case("pool 256, shared outputs behind it", 9, &fill, [](P *p, int last) { p[last].cus = p[0].cus; p[last].rec_y = p[0].rec_y; p[last].dst_y = p[0].dst_y; });
  filter_case("record 1 before record 2", 3, [](P *p) { p[1].lcu_last_qp = p[0].lcu_last_qp; p[1].rec_y = p[0].rec_y; p[1].stats = p[0].stats; p[1].dst_y = p[0].dst_y; p[2].deblock.chroma = 0; });

  // ---- kvz_hip_inter_recon_frames ----
  recon_case("clean", [](R *, Q *, int &) {});
  // what tests/test_gpu_inter_recon_multi.py plants, at the indices it plants them
  recon_case("refs[1] 5", [](R *p, Q *, int &) { p[2].refs[1] = 5; });
  recon_case("refs[0] 255", [](R *p, Q *, int &) { p[1].refs[0] = 255; });
  recon_case("pool 3 width 72", [](R *, Q *q, int &) { q[3].width = 72; });
  recon_case("pool 1 height 56", [](R *, Q *q, int &) { q[1].height = 56; });
  recon_case("pool 2 without u", [](R *, Q *q, int &) { q[2].u = nullptr; });
  recon_case("pool 0 without v", [](R *, Q *q, int &) { q[0].v = nullptr; });
  recon_case("pool 4 without y", [](R *, Q *q, int &) { q[4].y = nullptr; });
  recon_case("n_refs 0", [](R *p, Q *, int &) { p[1].params.n_refs = 0; });
  recon_case("n_refs 17", [](R *p, Q *, int &) { p[2].params.n_refs = 17; });
  recon_case("width 60", [](R *p, Q *, int &) { p[0].width = 60; });
  recon_case("height 36", [](R *p, Q *, int &) { p[2].height = 36; });
  recon_case("stride_y 56", [](R *p, Q *, int &) { p[1].stride_y = 56; });
  recon_case("stride_c 24", [](R *p, Q *, int &) { p[0].stride_c = 24; });
  recon_case("cus + 2", [](R *p, Q *, int &) { p[2].cus = plus(p[2].cus, 2); });
  recon_case("cus null", [](R *p, Q *, int &) { p[1].cus = nullptr; });
  recon_case("pred_y null", [](R *p, Q *, int &) { p[0].pred_y = nullptr; });
  recon_case("pred_u null", [](R *p, Q *, int &) { p[1].pred_u = nullptr; });
  recon_case("pred_y of record 0", [](R *p, Q *, int &) { p[2].pred_y = p[0].pred_y; });
  recon_case("pred_y is pool 4 y", [](R *p, Q *q, int &) { p[1].pred_y = const_cast<kvz_hip_pixel *>(q[4].y); });
  recon_case("pred_v is pool 3 v", [](R *p, Q *q, int &) { p[0].pred_v = const_cast<kvz_hip_pixel *>(q[3].v); });
  // what is accepted
  recon_case("255 behind n_refs, a garbage slot, no chroma under 4:0:0", [](R *p, Q *q, int &n_pool) {
    for (int i = 0; i < 3; ++i)
      for (int k = 2; k < 16; ++k) p[i].refs[k] = 255;
    q[4].u = q[4].v = nullptr;
    q[5] = Q{ nullptr, nullptr, nullptr, 0, 0, 60, 7 };
    n_pool = 6;
  });
  recon_case("odd planes", [](R *p, Q *q, int &) { p[0].pred_y = plus(p[0].pred_y, 1); p[0].stride_y = 67; p[0].pred_v = plus(p[0].pred_v, 3); q[1].y = plus(q[1].y, 1); });
  recon_case("pred_u is pool 4 u under 4:0:0", [](R *p, Q *q, int &) { p[2].pred_u = const_cast<kvz_hip_pixel *>(q[4].u); });
  recon_case("pred_y is the y of a pool picture that nobody names", [](R *p, Q *q, int &n_pool) { q[5] = pool_picture(5, 64, 64); n_pool = 6; p[0].pred_y = const_cast<kvz_hip_pixel *>(q[5].y); });
  // two defects: the first check in the entry's order names the reason
  recon_case("cus null, width 60", [](R *p, Q *, int &) { p[1].cus = nullptr; p[1].width = 60; });
  recon_case("width 60, n_refs 0", [](R *p, Q *, int &) { p[1].width = 60; p[1].params.n_refs = 0; });
  recon_case("n_refs 17, pred_u null", [](R *p, Q *, int &) { p[1].params.n_refs = 17; p[1].pred_u = nullptr; });
  recon_case("pred_u null, refs[0] 255", [](R *p, Q *, int &) { p[1].pred_u = nullptr; p[1].refs[0] = 255; });
  recon_case("refs[0] 255, pool 3 width 72", [](R *p, Q *q, int &) { p[1].refs[0] = 255; q[3].width = 72; });
  recon_case("pool 2 width 72, refs[1] 255", [](R *p, Q *q, int &) { q[2].width = 72; p[1].refs[1] = 255; });
  recon_case("pool 3 width 72, pred_y of record 0", [](R *p, Q *q, int &) { q[3].width = 72; p[1].pred_y = p[0].pred_y; });
  // 2^30 workgroups each: the second such picture exceeds the grid
  const auto huge = [](R *p, Q *q) {
    for (int i = 1; i < 3; ++i) { p[i] = recon_picture(i, 1 << 20, 1 << 20, 0, 4, 4); }
    q[4] = pool_picture(4, 1 << 20, 1 << 20);
  };
  recon_case("two huge pictures", [&](R *p, Q *q, int &) { huge(p, q); });
  recon_case("one huge picture", [&](R *p, Q *q, int &) { huge(p, q); p[1] = recon_picture(1, 64, 64, 1, 2, 3); });
  recon_case("pred_y of record 0, two huge pictures", [&](R *p, Q *q, int &) { huge(p, q); p[2].pred_y = p[0].pred_y; });
  recon_case("two huge pictures, pred_y is pool 1 y", [&](R *p, Q *q, int &) { huge(p, q); p[0].pred_y = const_cast<kvz_hip_pixel *>(q[1].y); });
  recon_case("record 1 before record 0's destination", [](R *p, Q *q, int &) { p[0].pred_y = const_cast<kvz_hip_pixel *>(q[4].y); p[1].cus = nullptr; });
  option_cases();
  return 0;
}
"""


def four(qp=None, deblock=None, stats=None, sao=None):
    return {"qp": qp, "deblock": deblock, "stats": stats, "sao": sao}


def tiled(v):
    """the three stages that take tiles"""
    return four(qp=v, deblock=v, sao=v)


def recon(v=None):
    return {"recon": v}


# case -> {stage: None where the call is accepted, else (index of the first refused record, reason)}
EXPECTED = {
    "clean": four(),
    "clean sixteen": four(),
    "deblock.chroma 0": four((2, CHROMA), (2, CHROMA), (2, CHROMA), (2, CHROMA)),
    "width - 4": four((2, QP_SIZE), (2, DEBLOCK), (2, SRC), (2, PLANES)),
    "height 4": four((2, QP_SIZE), (2, DEBLOCK), (2, SRC), (2, PLANES)),
    "cus null": four(qp=(2, QP_PTR), deblock=(2, DEBLOCK)),
    "cbf null": four(qp=(2, QP_PTR)),
    "lcu_qp null": four(qp=(2, QP_PTR)),
    "lcu_last_qp null": four(qp=(2, QP_PTR)),
    "rec_y null": four(deblock=(2, DEBLOCK), stats=(2, PLANES), sao=(2, PLANES)),
    "rec_u null": four(deblock=(2, DEBLOCK), stats=(2, CHROMA_PLANE), sao=(2, SAO_CHROMA)),
    "stats null": four(stats=(2, STATS_OUT)),
    "src.y null": four(stats=(2, PLANES)),
    "src.v null": four(stats=(2, CHROMA_PLANE)),
    "sao_luma null": four(sao=(2, SAO_LUMA)),
    "sao_chroma null": four(sao=(2, SAO_CHROMA)),
    "dst_y null": four(sao=(2, PLANES)),
    "dst_v null": four(sao=(2, SAO_CHROMA)),
    "cus + 2": four(qp=(2, QP_PTR), deblock=(2, DEBLOCK)),
    "rec_y + 1": four(deblock=(2, DEBLOCK), stats=(2, PLANES), sao=(2, PLANES)),
    "stats + 2": four(stats=(2, STATS_OUT)),
    "cands + 1": four(stats=(2, STATS_OUT)),
    "src.width + 8": four(stats=(2, SRC)),
    "sao_luma + 2": four(sao=(2, SAO_LUMA)),
    "stride_y - 4": four(deblock=(2, DEBLOCK), stats=(2, PLANES), sao=(2, PLANES)),
    "src.stride_y - 4": four(stats=(2, PLANES)),
    "dst_stride_y - 4": four(sao=(2, PLANES)),
    "stride_c - 4": four(deblock=(2, DEBLOCK), stats=(2, CHROMA_PLANE), sao=(2, SAO_CHROMA)),
    "dst_y is rec_y": four(sao=(2, SAO_LUMA)),
    "dst_u is rec_u": four(sao=(2, SAO_CHROMA)),
    "cus of record 0": four(qp=(2, SHARED)),                  # the SCU map is an input of deblocking
    "lcu_last_qp of record 1": four(qp=(2, SHARED)),
    "rec_y of record 0": four(deblock=(2, SHARED)),           # the rec planes are inputs of the statistics and of SAO
    "stats of record 1": four(stats=(2, SHARED)),
    "dst_y of record 0": four(sao=(2, SHARED)),
    "ragged grid": four(),
    "start_qp -1": four(qp=(2, QP_CHAIN)),
    "start_qp 52": four(qp=(2, QP_CHAIN)),
    "start_qp 0 and 51": four(),
    "chain_rows 2": four(qp=(2, QP_CHAIN)),
    "chain_rows -1": four(qp=(2, QP_CHAIN)),
    "chain_rows 1": four(),
    "cus null in the middle": four(qp=(1, QP_PTR), deblock=(1, DEBLOCK)),
    "pool 260": tiled((9, POOL)),                             # the statistics take no grid
    "pool 256": four(),
    "4:0:0 without chroma planes": four(),
    "cands null": four(),
    "cands null in two records": four(),
    "cands of record 0": four(stats=(2, SHARED)),
    "shared inputs": four(),
    "width 16384": four(),
    "width 16392": four((1, QP_SIZE), (1, DEBLOCK), (1, PLANES), (1, PLANES)),
    "cus null, width - 4": four((1, QP_PTR), (1, DEBLOCK), (1, PLANES), (1, PLANES)),
    "width - 4, start_qp 52": four((1, QP_SIZE), (1, DEBLOCK), (1, PLANES), (1, PLANES)),
    "start_qp 52, deblock.chroma 0": four((1, QP_CHAIN), (1, CHROMA), (1, CHROMA), (1, CHROMA)),
    "deblock.chroma 0, bad grid": four((2, CHROMA), (2, CHROMA), (2, CHROMA), (2, CHROMA)),
    "deblock.chroma 0, src.width + 8": four((2, CHROMA), (2, CHROMA), (2, CHROMA), (2, CHROMA)),
    "deblock.chroma 0, sao_luma null, rec_y + 1": four((2, CHROMA), (2, CHROMA), (2, CHROMA), (2, CHROMA)),
    "src.width + 8, stats null": four(stats=(2, SRC)),
    "stats null, sao_luma null, rec_y null": four(deblock=(2, DEBLOCK), stats=(2, STATS_OUT), sao=(2, SAO_LUMA)),
    "rec_y + 1, rec_u null, sao_chroma null": four(deblock=(2, DEBLOCK), stats=(2, PLANES), sao=(2, PLANES)),
    "rec_u null, bad grid, stats of record 0": four((2, GRID), (2, DEBLOCK), (2, CHROMA_PLANE), (2, SAO_CHROMA)),
    "bad grid, shared outputs": tiled((2, GRID)),
    "bad grid where the pool is full": tiled((9, GRID)),
    "pool 260, shared outputs": tiled((9, POOL)),
    "pool 256, shared outputs behind it": tiled((10, SHARED)),
    "record 1 before record 2": four((1, SHARED), (1, SHARED), (1, SHARED), (1, SHARED)),
}
EXPECTED.update({"bad grid %d" % k: tiled((2, GRID)) for k in range(12)})
EXPECTED.update({"recon " + name: recon(v) for name, v in {
    "clean": None,
    "refs[1] 5": (2, R_INDEX),
    "refs[0] 255": (1, R_INDEX),
    "pool 3 width 72": (1, R_REF),
    "pool 1 height 56": (0, R_REF),
    "pool 2 without u": (1, R_REF),
    "pool 0 without v": (0, R_REF),
    "pool 4 without y": (2, R_REF),
    "n_refs 0": (1, R_NREFS),
    "n_refs 17": (2, R_NREFS),
    "width 60": (0, R_SIZE),
    "height 36": (2, R_SIZE),
    "stride_y 56": (1, R_SIZE),
    "stride_c 24": (0, R_CHROMA),
    "cus + 2": (2, R_PTR),
    "cus null": (1, R_PTR),
    "pred_y null": (0, R_PTR),
    "pred_u null": (1, R_CHROMA),
    "pred_y of record 0": (2, R_SHARED),
    "pred_y is pool 4 y": (1, R_DST),
    "pred_v is pool 3 v": (0, R_DST),
    "255 behind n_refs, a garbage slot, no chroma under 4:0:0": None,
    "odd planes": None,
    "pred_u is pool 4 u under 4:0:0": None,
    "pred_y is the y of a pool picture that nobody names": None,
    "cus null, width 60": (1, R_PTR),
    "width 60, n_refs 0": (1, R_SIZE),
    "n_refs 17, pred_u null": (1, R_NREFS),
    "pred_u null, refs[0] 255": (1, R_CHROMA),
    "refs[0] 255, pool 3 width 72": (1, R_INDEX),
    "pool 2 width 72, refs[1] 255": (1, R_REF),               # reference 0 is looked at in full before reference 1
    "pool 3 width 72, pred_y of record 0": (1, R_REF),
    "two huge pictures": (2, R_GRID),
    "one huge picture": None,
    "pred_y of record 0, two huge pictures": (2, R_SHARED),
    "two huge pictures, pred_y is pool 1 y": (2, R_GRID),     # the destinations are looked at after all records
    "record 1 before record 0's destination": (1, R_PTR),
}.items()})

# the predicates and the packing: True where accepted
OPTIONS = {
    "deblock single 16392": True,
    "deblock record 16392": False,
    "cu_qp size 16392": False,
    "sao luma planes 16392": False,
    "recon odd planes": True,
    "recon odd reference": True,
    "sao odd rec_y": False,
    "recon size 16392": True,
    "cu_qp pack without params": False,
    "deblock pack without params": False,
    "sao_stats pack without src": False,
    "inter_recon pack without refs": False,
    "inter_recon pack without params": False,
}
OPTIONS.update({"record %d packed by %s" % (i, entry): True for i in range(3)
                for entry in ("cu_qp", "deblock", "sao_stats", "sao", "inter_recon")})


@functools.lru_cache(maxsize=None)
def program_output():
    """the program's lines, compiled and run once: ({case: {stage: verdict}}, {option: accepted})"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "filter_host_checks.cpp"), os.path.join(tmp, "filter_host_checks")
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
        if stage == "recon":
            name = "recon " + name
        got.setdefault(name, {})[stage] = None if verdict == "ok" else (int(index), reason)
    return got, options


def test_record_checks_report_the_first_refused_record_and_its_reason():
    got, _ = program_output()
    assert sorted(got) == sorted(EXPECTED)
    for name, want in EXPECTED.items():
        assert got[name] == want, name


def test_single_entry_predicates_and_the_records_of_the_single_picture_entries():
    _, options = program_output()
    assert sorted(options) == sorted(OPTIONS)
    for name, accepted in OPTIONS.items():
        assert options[name] == accepted, name

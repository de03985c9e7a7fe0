// chain_host.h -- the host side that the entries of the picture chain share, single-picture and multi-picture alike: the residual
// stages (kvz_hip_inter_residual_*, kvz_hip_intra_recon_*), the filter stages (kvz_hip_cu_qp_*, kvz_hip_deblock_*, kvz_hip_sao_stats_*,
// kvz_hip_sao_*), motion compensation (kvz_hip_inter_recon_*) and the hash stage (kvz_hip_picture_hash_frame(s),
// kvz_hip_array_checksum_batch): the refusal that names a record, the prologue on the record count, the size and plane rules, the tile
// grid on the host with the pool of boundaries of a call, and per stage the rules of one picture as predicates on the stage's record,
// the pack of a single-picture entry's arguments into that record, why a record of a call is refused, and the walk over the records
// of a call (chain_records_why with the launch plan, filter_records_why, recon_records_why).  Each rule is written once.
//
// Host only: pointer and integer arithmetic on the structs of kvz_hip.h, which compare pointers and never follow them (a
// kvz_hip_tile_grid, a kvz_hip_trskip and the pool of reference pictures are host memory and are read).  No device code and no HIP call,
// so a plain C++17 compiler takes this header with kvz_hip.h alone (tests/test_chain_host_checks.py, test_filter_host_checks.py and
// test_picture_hash_abi.py run the record checks that way, without a device).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/kvz_hip.h"

namespace kvzhip {
void set_error_msg(const char *what);           // api.hip
}

namespace {

// ---- refusing record i of a call; i < 0 (refuse_entry): a single-picture entry's refusal under a text of its own ----
inline int refuse_picture(const char *entry, int i, const char *why)
{
  char msg[200];
  if (i < 0) snprintf(msg, sizeof msg, "%s: %s", entry, why);
  else snprintf(msg, sizeof msg, "%s: invalid argument in picture %d (%s)", entry, i, why);
  kvzhip::set_error_msg(msg);
  return KVZ_HIP_ERR_INVALID;
}
inline int refuse_entry(const char *entry, const char *why) { return refuse_picture(entry, -1, why); }

// How every multi-picture entry begins: a context, no pictures is a no-op, and the count in range (KVZ_CHECK_CTX, kvz_hip_internal.h)
#define KVZ_CHAIN_PROLOGUE(pictures, n_pictures)                                                                               \
  KVZ_CHECK_CTX();                                                                                                             \
  if ((n_pictures) == 0) return KVZ_HIP_OK;                                                                                    \
  if (!(pictures) || (n_pictures) < 0 || (n_pictures) > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__)

// ---- the size rule and the plane rule ----
// no upper bound: the single deblocking entries and motion compensation, which carry a size in an int and never in a record's 16 bits
inline bool picture_ok_any_size(int width, int height) { return width >= 8 && height >= 8 && !((width | height) & 7); }
// width / height: multiples of 8 (the minimum CU) in 8..16384
inline bool picture_ok(int width, int height) { return picture_ok_any_size(width, height) && width <= 16384 && height <= 16384; }
// no alignment: motion compensation, whose kernels read their windows at any byte offset and so ask nothing of a plane's base
inline bool plane_ok_unaligned(const void *p, uint32_t stride, int w) { return p && stride >= (uint32_t)w; }
// a plane that is read or written by the dword: 4-byte aligned base and stride, stride >= the width
inline bool plane_ok(const void *p, uint32_t stride, int w) { return plane_ok_unaligned(p, stride, w) && !((uintptr_t)p & 3) && !(stride & 3); }
// the u and v planes of a 4:2:0 picture, which share a stride
inline bool chroma_planes_ok(const void *u, const void *v, uint32_t stride_c, int w) { return plane_ok(u, stride_c, w >> 1) && plane_ok(v, stride_c, w >> 1); }

// ---- the tile grid on the host ----
static_assert(sizeof(kvz_hip_tile_grid) == 392 && KVZ_HIP_MAX_TILES_PER_DIM == 48, "layout documented in kvz_hip.h");

constexpr int TILE_MAX = KVZ_HIP_MAX_TILES_PER_DIM - 1;      // the largest count of tile columns or rows

inline bool tile_bd_ok(int n, const int32_t *bd, int lcus)
{
  if (n < 1 || n > TILE_MAX || bd[0] != 0 || bd[n] != lcus) return false;
  for (int i = 0; i < n; ++i)
    if (bd[i + 1] <= bd[i]) return false;
  return true;
}

// grid == NULL: one tile, the whole picture.  -> false for a malformed grid (tiles_col_bd / tiles_row_bd, encoder.c:472-481)
inline bool tile_grid_make(const kvz_hip_tile_grid *grid, int width, int height, kvz_hip_tile_grid *out)
{
  const int lcus_x = (width + 63) >> 6, lcus_y = (height + 63) >> 6;
  __builtin_memset(out, 0, sizeof *out);
  if (!grid) {
    out->cols = out->rows = 1;
    out->col_bd[1] = lcus_x;
    out->row_bd[1] = lcus_y;
    return true;
  }
  if (!tile_bd_ok(grid->cols, grid->col_bd, lcus_x) || !tile_bd_ok(grid->rows, grid->row_bd, lcus_y)) return false;
  // the entries beyond the counts are not the caller's to define: they travel as zeros
  out->cols = grid->cols;
  out->rows = grid->rows;
  for (int i = 0; i <= grid->cols; ++i) out->col_bd[i] = grid->col_bd[i];
  for (int i = 0; i <= grid->rows; ++i) out->row_bd[i] = grid->row_bd[i];
  return true;
}

// the largest tile's wavefront count w + 2 (h - 1): the dependent launches of the intra stage
inline int tile_grid_waves(const kvz_hip_tile_grid &g)
{
  int w = 0, h = 0;
  for (int i = 0; i < g.cols; ++i) w = g.col_bd[i + 1] - g.col_bd[i] > w ? g.col_bd[i + 1] - g.col_bd[i] : w;
  for (int i = 0; i < g.rows; ++i) h = g.row_bd[i + 1] - g.row_bd[i] > h ? g.row_bd[i + 1] - g.row_bd[i] : h;
  return w + 2 * (h - 1);
}

// ---- the grids of the pictures of a multi-picture call ----
// Sixteen kvz_hip_tile_grid do not fit the kernel arguments; the boundaries that a call uses do: one pool of KVZ_HIP_CHAIN_TILE_BOUNDS
// 16-bit values (an LCU index is at most 256) that the records share, two to a dword (tile_pool, tile_grid.h; intra_batch_ts_data,
// intra_recon_core.h).  A picture's record says where its cols + 1 column and rows + 1 row boundaries stand.  A picture without a grid
// is one tile and takes nothing from the pool: the first boundary is 0 and the last is the picture's LCU count, so only the boundaries
// between them are ever read.
struct pic_tiles { uint16_t col_at, row_at, lcus_x, lcus_y; uint8_t cols, rows, pad[2]; };
static_assert(sizeof(pic_tiles) == 12, "kernel arguments");

// -> false where the pool is full.  g: what tile_grid_make made of grid
inline bool tile_pool_add(const kvz_hip_tile_grid *grid, const kvz_hip_tile_grid &g, uint16_t *bounds, int &used, pic_tiles *t)
{
  __builtin_memset(t, 0, sizeof *t);
  t->cols = (uint8_t)g.cols; t->rows = (uint8_t)g.rows;
  t->lcus_x = (uint16_t)g.col_bd[g.cols]; t->lcus_y = (uint16_t)g.row_bd[g.rows];
  if (!grid) return true;
  if (used + g.cols + g.rows + 2 > KVZ_HIP_CHAIN_TILE_BOUNDS) return false;
  t->col_at = (uint16_t)used;
  for (int j = 0; j <= g.cols; ++j) bounds[used++] = (uint16_t)g.col_bd[j];
  t->row_at = (uint16_t)used;
  for (int j = 0; j <= g.rows; ++j) bounds[used++] = (uint16_t)g.row_bd[j];
  return true;
}
inline void tile_pool_pack(const uint16_t *bounds, int used, uint32_t (&bd)[KVZ_HIP_CHAIN_TILE_BOUNDS / 2])
{
  __builtin_memset(bd, 0, sizeof bd);
  for (int j = 0; j < used; ++j) bd[j >> 1] |= (uint32_t)bounds[j] << (16 * (j & 1));
}

// ---- one picture of a residual stage ----
// what every entry requires of one picture's arguments, the QP and the tables aside; intra: the entry reads intra_modes; lists: the
// entry takes scaling lists
inline bool chain_picture_args_ok(const kvz_hip_chain_picture &p, bool intra, bool lists)
{
  if (!p.rec_y || !p.cus || (intra && !p.intra_modes) || !p.coeff_y || !p.src.y || ((uintptr_t)p.cus & 3) || ((uintptr_t)p.coeff_y & 15) ||
      ((uintptr_t)p.costs & 3))
    return false;
  const int width = p.src.width, height = p.src.height;
  if (!picture_ok(width, height) || p.stride_y < (uint32_t)width || p.src.stride_y < (uint32_t)width || (p.params.scaling_list != 0) != lists)
    return false;
  if (p.params.chroma && (!p.rec_u || !p.rec_v || !p.coeff_u || !p.coeff_v || !p.src.u || !p.src.v || p.stride_c < (uint32_t)(width >> 1) ||
                          p.src.stride_c < (uint32_t)(width >> 1) || (((uintptr_t)p.coeff_u | (uintptr_t)p.coeff_v) & 15)))
    return false;
  return true;
}
// The single-picture entries take the fields as loose arguments: each packs them once into the record that kvz_hip.h says they are,
// and everything behind the entry reads the record.  -> false without src or params, which are copied
inline bool chain_picture_pack(kvz_hip_chain_picture *p, const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                               kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes, kvz_hip_coeff *coeff_y,
                               kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp,
                               const kvz_hip_inter_residual_params *params)
{
  if (!src || !params) return false;
  *p = { *src, rec_y, rec_u, rec_v, stride_y, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, *params };
  return true;
}

// ---- one check per option, for the single-picture entries and the records of a call alike ----
// scaling lists: both tables, 16-byte aligned (a lane reads its row of each with 16-byte loads)
inline bool chain_tables_ok(const kvz_hip_scaling_tables &t)
{
  return t.quant && t.dequant && !(((uintptr_t)t.quant | (uintptr_t)t.dequant) & 15);
}
// transform skip, ts != NULL: the array of choices, and a bit cost that is an aligned array or one value that is not negative
inline bool chain_trskip_ok(const kvz_hip_trskip *ts, const uint8_t *tr_skip_out)
{
  return tr_skip_out && (ts->lcu_bit_cost || ts->bit_cost >= 0) && !((uintptr_t)ts->lcu_bit_cost & 3);
}
// RDOQ, rdoq != NULL (kvz_hip_inter_residual_frame_rdoq, kvz_hip_intra_recon_frame_rdoq): why the record is refused, or nullptr.  The
// order of the checks is part of the interface (tests/test_rdoq_chain_host_checks.py pins it)
inline const char *chain_rdoq_why(const kvz_hip_rdoq_source *r)
{
  if (!r->ctx_sets || !r->states) return "ctx_sets or states is null";
  if (!r->tables.quant || !r->tables.err_scale) return "a table is null";
  if (r->n_sets == 0) return "n_sets is 0";
  if (((uintptr_t)r->ctx_sets & 1) || ((uintptr_t)r->lcu_ctx & 1)) return "ctx_sets or lcu_ctx not 2-byte aligned";
  if (((uintptr_t)r->states & 7) || ((uintptr_t)r->tables.err_scale & 7)) return "states or err_scale not 8-byte aligned";
  if ((uintptr_t)r->tables.quant & 15) return "quant not 16-byte aligned";
  return nullptr;
}
// the text under which a single-picture entry refuses for that reason: refuse_entry(__func__, invalid_because(why).text)
struct refusal_text { char text[200]; };
inline refusal_text invalid_because(const char *why)
{
  refusal_text t;
  snprintf(t.text, sizeof t.text, "invalid argument (%s)", why);
  return t;
}
// one QP for the picture (no lcu_qp): what the one-QP entry refuses.  That entry asks make_consts (quant_core.h) for the constants of
// the 4x4 luma and chroma TUs, which fails where scaled_qp is negative: for luma that is the QP itself, for chroma it is clamped into
// 0..57 (tests/test_chain_host_checks.py holds this rule against what make_consts decided for every QP)
inline bool chain_one_qp_ok(const kvz_hip_chain_picture &p) { return p.lcu_qp || p.params.qp >= 0; }

// ---- the records of a call: why record i is refused, or nullptr.  The order of the checks is part of the interface: it decides
// which reason a record with two defects reports (tests/test_chain_host_checks.py pins it). ----

// the outputs whose base pointers two records must not share
inline bool chain_output_shared(const kvz_hip_chain_picture &p, const kvz_hip_chain_picture &o)
{
  return p.rec_y == o.rec_y || p.cus == o.cus || p.coeff_y == o.coeff_y;
}

// kvz_hip_inter_residual_frames / kvz_hip_intra_recon_frames: one reason for everything
inline const char *chain_record_why(const kvz_hip_chain_picture *pictures, int i, bool intra)
{
  const char *const why = "null or misaligned buffer, size or parameter out of range, or an output shared with another picture";
  const kvz_hip_chain_picture &p = pictures[i];
  if (!chain_picture_args_ok(p, intra, false) || !chain_one_qp_ok(p)) return why;
  for (int j = 0; j < i; ++j)
    if (chain_output_shared(p, pictures[j])) return why;
  return nullptr;
}

// kvz_hip_inter_residual_frames_ts / kvz_hip_intra_recon_frames_ts; lists, skip: what record 0 carries.  The record's own checks, then
// (chain_record_ts_shared) the earlier records: the intra entry checks the record's tile grid between the two
inline const char *chain_record_ts_why(const kvz_hip_chain_picture_ts *pictures, int i, bool intra, bool lists, bool skip)
{
  const kvz_hip_chain_picture_ts &r = pictures[i];
  const kvz_hip_chain_picture &p = r.pic;
  const bool has_lists = r.tables.quant || r.tables.dequant;
  if (has_lists != lists || (r.ts != nullptr) != skip)
    return "a call is homogeneous: every record carries tables or none does, every record carries ts or none does";
  if (has_lists && !chain_tables_ok(r.tables)) return "a table is null or not 16-byte aligned";
  if (!chain_picture_args_ok(p, intra, has_lists))
    return "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given";
  if (r.ts && !chain_trskip_ok(r.ts, r.tr_skip_out)) return "ts without tr_skip_out, a negative bit_cost without lcu_bit_cost, or a misaligned lcu_bit_cost";
  if (!chain_one_qp_ok(p)) return "a negative qp without lcu_qp";
  return nullptr;
}
inline const char *chain_record_ts_shared(const kvz_hip_chain_picture_ts *pictures, int i)
{
  const kvz_hip_chain_picture_ts &r = pictures[i];
  for (int j = 0; j < i; ++j)
    if (chain_output_shared(r.pic, pictures[j].pic) || (r.ts && r.tr_skip_out == pictures[j].tr_skip_out)) return "an output shared with another picture";
  return nullptr;
}

// kvz_hip_inter_residual_frames_rdoq / kvz_hip_intra_recon_frames_rdoq; lists: record 0 carries tables, skip: record 0's rdoq_skip (not
// read where record 0 carries no rdoq).  Homogeneity comes first, as in chain_record_ts_why, so the kernel that would run is known
// before a record is looked into: the presence of tables and of rdoq, then the three values that the records of a call share.  Then
// the record's own checks -- tables, the picture, chain_rdoq_why, the QP; then (chain_record_rdoq_shared) the earlier records: the
// intra entry checks the record's tile grid between the two
static_assert(sizeof(kvz_hip_chain_picture_rdoq) == 192 && sizeof(kvz_hip_rdoq_source) == 48, "layout documented in kvz_hip.h");
inline const char *chain_record_rdoq_why(const kvz_hip_chain_picture_rdoq *pictures, int i, bool intra, bool lists, bool skip)
{
  const kvz_hip_chain_picture_rdoq &r = pictures[i];
  const kvz_hip_rdoq_source *first = pictures[0].rdoq;
  const bool has_lists = r.tables.quant || r.tables.dequant;
  if (has_lists != lists || (r.rdoq != nullptr) != (first != nullptr))
    return "a call is homogeneous: every record carries tables or none does, every record carries rdoq or none does";
  if (r.rdoq && ((r.rdoq->rdoq_skip != 0) != skip || r.rdoq->tables.quant != first->tables.quant || r.rdoq->tables.err_scale != first->tables.err_scale))
    return "a call is homogeneous: rdoq_skip, rdoq->tables.quant and rdoq->tables.err_scale are those of record 0";
  if (has_lists && !chain_tables_ok(r.tables)) return "a table is null or not 16-byte aligned";
  if (!chain_picture_args_ok(r.pic, intra, has_lists))
    return "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given";
  if (r.rdoq)
    if (const char *why = chain_rdoq_why(r.rdoq)) return why;
  if (!chain_one_qp_ok(r.pic)) return "a negative qp without lcu_qp";
  return nullptr;
}
inline const char *chain_record_rdoq_shared(const kvz_hip_chain_picture_rdoq *pictures, int i)
{
  for (int j = 0; j < i; ++j)
    if (chain_output_shared(pictures[i].pic, pictures[j].pic)) return "an output shared with another picture";
  return nullptr;
}

// ---- the records of a call of either residual stage, all checked before anything is launched ----
// The three record types differ in how the picture and the grid are reached, and in which checks are theirs (chain_own_why takes
// lists and skip from record 0).  kvz_hip_chain_picture has one reason for everything, the earlier records included, and never a grid.
inline const kvz_hip_chain_picture &chain_pic(const kvz_hip_chain_picture &r) { return r; }
inline const kvz_hip_chain_picture &chain_pic(const kvz_hip_chain_picture_ts &r) { return r.pic; }
inline const kvz_hip_chain_picture &chain_pic(const kvz_hip_chain_picture_rdoq &r) { return r.pic; }
inline const kvz_hip_tile_grid *chain_grid(const kvz_hip_chain_picture &) { return nullptr; }
inline const kvz_hip_tile_grid *chain_grid(const kvz_hip_chain_picture_ts &r) { return r.grid; }
inline const kvz_hip_tile_grid *chain_grid(const kvz_hip_chain_picture_rdoq &r) { return r.grid; }
inline const char *chain_own_why(const kvz_hip_chain_picture *pictures, int i, bool intra) { return chain_record_why(pictures, i, intra); }
inline const char *chain_own_why(const kvz_hip_chain_picture_ts *pictures, int i, bool intra)
{
  return chain_record_ts_why(pictures, i, intra, pictures[0].tables.quant || pictures[0].tables.dequant, pictures[0].ts != nullptr);
}
inline const char *chain_own_why(const kvz_hip_chain_picture_rdoq *pictures, int i, bool intra)
{
  const kvz_hip_rdoq_source *first = pictures[0].rdoq;
  return chain_record_rdoq_why(pictures, i, intra, pictures[0].tables.quant || pictures[0].tables.dequant, first && first->rdoq_skip != 0);
}
inline const char *chain_shared_why(const kvz_hip_chain_picture *, int) { return nullptr; }
inline const char *chain_shared_why(const kvz_hip_chain_picture_ts *pictures, int i) { return chain_record_ts_shared(pictures, i); }
inline const char *chain_shared_why(const kvz_hip_chain_picture_rdoq *pictures, int i) { return chain_record_rdoq_shared(pictures, i); }

// the grids of an intra call: the pool of boundaries as tile_pool_pack takes it, and every picture's place in it
struct chain_tiles { uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS]; int used; pic_tiles pic[KVZ_HIP_MAX_CHAIN_PICTURES]; };
// What the records ask of the launches.  init_scus: the SCUs of the largest picture that has cbf_out or costs, 0 where none has: the
// init launch.  The intra stage: the largest tile's wavefront count, a workgroup per LCU row and tile column of the picture with the
// most, and three planes where a picture has chroma.  The inter stage sizes its launches of the kernel's records (launch_pictures).
struct chain_plan { int init_scus, waves, groups, planes; };

// Per record: its own checks, homogeneity first; for the intra stage its grid, and the grid's place in the pool (tiles); then its
// outputs against those of the earlier records.  The inter stage does not depend on tiles: it never looks at a grid, and tiles is
// not read.  The order is part of the interface (tests/test_chain_host_checks.py and test_chain_multi_rdoq_host_checks.py run this
// function).  -> the reason, with *at the record that is refused, or nullptr
template <typename RECORD>
inline const char *chain_records_why(const RECORD *pictures, int n, bool intra, chain_tiles *tiles, chain_plan *plan, int *at)
{
  *plan = { 0, 0, 0, 1 };
  if (intra) tiles->used = 0;
  for (int &i = *at = 0; i < n; ++i) {
    const kvz_hip_chain_picture &p = chain_pic(pictures[i]);
    if (const char *w = chain_own_why(pictures, i, intra)) return w;
    if (intra) {
      // a record without a grid is one tile of lcus_x x lcus_y LCUs: lcus_x + 2 (lcus_y - 1) waves, lcus_y workgroups
      const kvz_hip_tile_grid *grid = chain_grid(pictures[i]);
      kvz_hip_tile_grid g;
      if (!tile_grid_make(grid, p.src.width, p.src.height, &g)) return "invalid tile grid";
      if (!tile_pool_add(grid, g, tiles->bounds, tiles->used, &tiles->pic[i])) return "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record";
      const int waves = tile_grid_waves(g), groups = (int)tiles->pic[i].lcus_y * g.cols;
      if (waves > plan->waves) plan->waves = waves;
      if (groups > plan->groups) plan->groups = groups;
      if (p.params.chroma) plan->planes = 3;
    }
    if (const char *w = chain_shared_why(pictures, i)) return w;
    const int scus = (p.src.width >> 2) * (p.src.height >> 2);
    if ((p.cbf_out || p.costs) && scus > plan->init_scus) plan->init_scus = scus;
  }
  return nullptr;
}

// ---- the hash stage: kvz_hip_picture_hash_frame(s) and kvz_hip_array_checksum_batch ----
static_assert(sizeof(kvz_hip_lcu_hash) == 24 && sizeof(kvz_hip_picture_hash) == 40 && sizeof(kvz_hip_hash_picture) == 104 &&
              sizeof(kvz_hip_hash_plane) == 24, "layout documented in kvz_hip.h");

// kvz_hip_picture_hash_frames, and kvz_hip_picture_hash_frame with its arguments as record 0
inline const char *hash_record_why(const kvz_hip_hash_picture *pictures, int i)
{
  const kvz_hip_hash_picture &p = pictures[i];
  const int width = p.width, height = p.height;
  if (!p.lcu_out || !p.out || ((uintptr_t)p.lcu_out & 3) || ((uintptr_t)p.out & 7)) return "lcu_out or out is null or misaligned";
  if (!picture_ok(width, height) || !plane_ok(p.rec_y, p.stride_y, width))
    return "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8";
  if (p.chroma && !chroma_planes_ok(p.rec_u, p.rec_v, p.stride_c, width))
    return "a chroma plane is null or misaligned, or its stride is";
  if (p.src.y) {
    if (p.src.width != width || p.src.height != height) return "src.width / src.height differ from width / height";
    if (!plane_ok(p.src.y, p.src.stride_y, width) || (p.chroma && !chroma_planes_ok(p.src.u, p.src.v, p.src.stride_c, width)))
      return "a src plane is null or misaligned, or its stride is";
  }
  for (int j = 0; j < i; ++j)
    if (p.lcu_out == pictures[j].lcu_out || p.out == pictures[j].out) return "an output shared with another picture";
  return nullptr;
}

// the 64 x 64 blocks of a plane of kvz_hip_array_checksum_batch; 0 for a size out of range
inline size_t hash_plane_blocks(int width, int height)
{
  if (width < 1 || height < 1 || width > 65536 || height > 65536) return 0;
  return (size_t)((width + 63) >> 6) * (size_t)((height + 63) >> 6);
}
inline const char *hash_plane_why(const kvz_hip_hash_plane &p)
{
  if (!p.data) return "data is null";
  if (!hash_plane_blocks(p.width, p.height)) return "width or height outside 1..65536";
  if (p.stride < (uint32_t)p.width) return "stride below the width";
  return nullptr;
}

// ---- the filter stages: the QP map, deblocking, the SAO statistics and SAO, on a kvz_hip_filter_picture ----
// A single-picture entry packs its loose arguments into the record that kvz_hip.h says they are (-> false without an argument that is
// copied) and composes the predicates of its stage under its own messages.  A multi-picture entry asks filter_records_why with the
// stage's X_record_why and X_output_shared: the order of the checks is part of the interface (tests/test_filter_host_checks.py).
typedef kvz_hip_filter_picture filter_pic;
inline const char *const PLANES_AND_STRIDES = "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8";
inline const char *filter_chroma_why(const filter_pic &p) { return p.deblock.chroma != p.chroma ? "deblock.chroma differs from chroma" : nullptr; }

// The records of a call, all checked before anything is launched: per record its own checks (why), for a stage that takes tiles its
// grid into the pool of boundaries (tiles[i]; tiles == NULL: the stage takes none), then its outputs against those of the earlier
// records (shared).  -> the reason, with *at the record that is refused, or nullptr
template <typename WHY, typename SHARED>
inline const char *filter_records_why(const filter_pic *pictures, int n, WHY why, SHARED shared, uint16_t *bounds, int &used, pic_tiles *tiles, int *at)
{
  for (int &i = *at = 0; i < n; ++i) {
    const filter_pic &p = pictures[i];
    kvz_hip_tile_grid g;
    if (const char *w = why(p)) return w;
    if (tiles && !tile_grid_make(p.grid, p.width, p.height, &g)) return "invalid tile grid";
    if (tiles && !tile_pool_add(p.grid, g, bounds, used, &tiles[i])) return "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record";
    for (int j = 0; j < i; ++j)
      if (shared(p, pictures[j])) return "an output shared with another picture";
  }
  return nullptr;
}

// -- the QP map.  kvz_hip_cu_qp_frame has raster runs for chains, which a record cannot say: it packs chain_rows 0 and keeps chain_lcus
inline bool cu_qp_pack(filter_pic *p, kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp, int8_t *lcu_last_qp,
                       const kvz_hip_tile_grid *grid, const kvz_hip_cu_qp_tiles_params *params)
{
  if (params) *p = { .width = width, .height = height, .cus = cus, .cbf = cbf, .lcu_qp = lcu_qp, .lcu_last_qp = lcu_last_qp, .grid = grid, .cu_qp = *params };
  return params != nullptr;
}
inline bool cu_qp_arrays_ok(const filter_pic &p) { return p.cus && p.cbf && p.lcu_qp && p.lcu_last_qp && !((uintptr_t)p.cus & 3); }
inline bool cu_qp_chains_ok(const filter_pic &p) { return p.cu_qp.start_qp >= 0 && p.cu_qp.start_qp <= 51 && (p.cu_qp.chain_rows == 0 || p.cu_qp.chain_rows == 1); }
inline const char *cu_qp_record_why(const filter_pic &p)
{
  if (!cu_qp_arrays_ok(p)) return "a null pointer or a misaligned cus";
  if (!picture_ok(p.width, p.height)) return "width / height must be multiples of 8 in 8..16384";
  if (!cu_qp_chains_ok(p)) return "start_qp outside 0..51 or chain_rows other than 0 and 1";
  return filter_chroma_why(p);
}
inline bool cu_qp_output_shared(const filter_pic &p, const filter_pic &o) { return p.cus == o.cus || p.lcu_last_qp == o.lcu_last_qp; }

// -- deblocking.  The single entries carry the size in an int and set no upper bound; the record check adds picture_ok, because the
// kernel's record stores width and height in 16 bits
inline bool deblock_pack(filter_pic *p, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, int width,
                         int height, const kvz_hip_cu_info *cus, const kvz_hip_tile_grid *grid, const kvz_hip_deblock_params *params)
{
  if (params) *p = { .width = width, .height = height, .chroma = params->chroma, .rec_y = rec_y, .rec_u = rec_u, .rec_v = rec_v, .stride_y = stride_y,
                     .stride_c = stride_c, .cus = const_cast<kvz_hip_cu_info *>(cus), .grid = grid, .deblock = *params };
  return params != nullptr;
}
inline bool deblock_luma_ok(const filter_pic &p) { return picture_ok_any_size(p.width, p.height) && plane_ok(p.rec_y, p.stride_y, p.width) && p.cus && !((uintptr_t)p.cus & 3); }
inline bool deblock_chroma_ok(const filter_pic &p) { return !p.chroma || chroma_planes_ok(p.rec_u, p.rec_v, p.stride_c, p.width); }
inline const char *deblock_record_why(const filter_pic &p)
{
  if (const char *why = filter_chroma_why(p)) return why;
  if (picture_ok(p.width, p.height) && deblock_luma_ok(p) && deblock_chroma_ok(p)) return nullptr;
  return "planes and the SCU map must be 4-byte aligned, width / height multiples of 8 in 8..16384, strides >= the width";
}
inline bool deblock_output_shared(const filter_pic &p, const filter_pic &o) { return p.rec_y == o.rec_y; }

// -- the SAO statistics
inline bool sao_stats_pack(filter_pic *p, const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                           const kvz_hip_pixel *rec_v, uint32_t stride_c, int chroma, kvz_hip_sao_lcu_stats *stats, kvz_hip_sao_lcu_cand *cands)
{
  if (src) *p = { .width = src->width, .height = src->height, .chroma = chroma, .src = *src, .rec_y = const_cast<kvz_hip_pixel *>(rec_y),
                  .rec_u = const_cast<kvz_hip_pixel *>(rec_u), .rec_v = const_cast<kvz_hip_pixel *>(rec_v), .stride_y = stride_y, .stride_c = stride_c,
                  .stats = stats, .cands = cands };
  return src != nullptr;
}
inline bool sao_stats_out_ok(const filter_pic &p) { return p.stats && !((uintptr_t)p.stats & 3) && !((uintptr_t)p.cands & 3); }
inline bool sao_stats_luma_ok(const filter_pic &p) { return picture_ok(p.width, p.height) && plane_ok(p.src.y, p.src.stride_y, p.width) && plane_ok(p.rec_y, p.stride_y, p.width); }
inline bool sao_stats_chroma_ok(const filter_pic &p)
{
  return !p.chroma || (chroma_planes_ok(p.src.u, p.src.v, p.src.stride_c, p.width) && chroma_planes_ok(p.rec_u, p.rec_v, p.stride_c, p.width));
}
inline const char *sao_stats_record_why(const filter_pic &p)
{
  if (const char *why = filter_chroma_why(p)) return why;
  if (p.src.width != p.width || p.src.height != p.height) return "src.width / src.height differ from width / height";
  if (!sao_stats_out_ok(p)) return "stats is null, or stats or cands misaligned";
  if (!sao_stats_luma_ok(p)) return PLANES_AND_STRIDES;
  return sao_stats_chroma_ok(p) ? nullptr : "a chroma plane is null or misaligned, or its stride is";
}
inline bool sao_stats_output_shared(const filter_pic &p, const filter_pic &o) { return p.stats == o.stats || (p.cands && p.cands == o.cands); }

// -- SAO: nothing that is copied, so its pack refuses nothing
inline void sao_pack(filter_pic *p, const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v, uint32_t stride_c,
                     kvz_hip_pixel *dst_y, uint32_t dst_stride_y, kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v, uint32_t dst_stride_c, int width, int height,
                     const kvz_hip_sao_info *sao_luma, const kvz_hip_sao_info *sao_chroma, int chroma, const kvz_hip_tile_grid *grid)
{
  *p = { .width = width, .height = height, .chroma = chroma, .rec_y = const_cast<kvz_hip_pixel *>(rec_y), .rec_u = const_cast<kvz_hip_pixel *>(rec_u),
         .rec_v = const_cast<kvz_hip_pixel *>(rec_v), .stride_y = stride_y, .stride_c = stride_c, .dst_y = dst_y, .dst_u = dst_u, .dst_v = dst_v,
         .dst_stride_y = dst_stride_y, .dst_stride_c = dst_stride_c, .sao_luma = sao_luma, .sao_chroma = sao_chroma, .grid = grid };
}
inline bool sao_luma_info_ok(const filter_pic &p) { return p.sao_luma && !((uintptr_t)p.sao_luma & 3) && p.dst_y != p.rec_y; }
inline bool sao_luma_planes_ok(const filter_pic &p) { return picture_ok(p.width, p.height) && plane_ok(p.rec_y, p.stride_y, p.width) && plane_ok(p.dst_y, p.dst_stride_y, p.width); }
inline bool sao_chroma_ok(const filter_pic &p)
{
  return !p.chroma || (p.sao_chroma && !((uintptr_t)p.sao_chroma & 3) && p.dst_u != p.rec_u && p.dst_v != p.rec_v &&
                       chroma_planes_ok(p.rec_u, p.rec_v, p.stride_c, p.width) && chroma_planes_ok(p.dst_u, p.dst_v, p.dst_stride_c, p.width));
}
inline const char *sao_record_why(const filter_pic &p)
{
  if (const char *why = filter_chroma_why(p)) return why;
  if (!sao_luma_info_ok(p)) return "sao_luma is null or misaligned, or dst_y is rec_y";
  if (!sao_luma_planes_ok(p)) return PLANES_AND_STRIDES;
  return sao_chroma_ok(p) ? nullptr : "sao_chroma or a chroma plane is null or misaligned, a chroma stride is, or a dst plane is its rec plane";
}
inline bool sao_output_shared(const filter_pic &p, const filter_pic &o) { return p.dst_y == o.dst_y; }

// ---- motion compensation, on a kvz_hip_recon_picture with its pool of reference pictures: no aligned planes, no size cap ----
// a table entry as the entries take it for a picture of width x height: chroma = the picture is 4:2:0
inline bool ref_ok(const kvz_hip_ref_picture &r, int chroma, int width, int height)
{
  if (r.width != width || r.height != height || !plane_ok_unaligned(r.y, r.stride_y, width)) return false;
  return !chroma || (plane_ok_unaligned(r.u, r.stride_c, width >> 1) && plane_ok_unaligned(r.v, r.stride_c, width >> 1));
}
inline bool refs_ok(const kvz_hip_ref_picture *refs, int n_refs, int chroma, int width, int height)
{
  for (int i = 0; i < n_refs; ++i)
    if (!ref_ok(refs[i], chroma, width, height)) return false;
  return true;
}
// kvz_hip_inter_recon_frame: its table is the pool, and reference i is pool picture i
inline bool recon_pack(kvz_hip_recon_picture *p, kvz_hip_pixel *pred_y, uint32_t stride_y, kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v, uint32_t stride_c,
                       int width, int height, const kvz_hip_cu_info *cus, const kvz_hip_ref_picture *refs, const kvz_hip_inter_recon_params *params)
{
  if (refs && params) *p = { .pred_y = pred_y, .pred_u = pred_u, .pred_v = pred_v, .stride_y = stride_y, .stride_c = stride_c, .width = width, .height = height,
                             .cus = cus, .refs = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, .params = *params };
  return refs && params;
}
inline bool recon_arrays_ok(const kvz_hip_recon_picture &p) { return p.pred_y && p.cus && !((uintptr_t)p.cus & 3); }
inline bool recon_luma_ok(const kvz_hip_recon_picture &p) { return picture_ok_any_size(p.width, p.height) && plane_ok_unaligned(p.pred_y, p.stride_y, p.width); }
inline bool recon_n_refs_ok(const kvz_hip_recon_picture &p) { return p.params.n_refs >= 1 && p.params.n_refs <= KVZ_HIP_MAX_REF_PICTURES; }
inline bool recon_chroma_ok(const kvz_hip_recon_picture &p)
{
  return !p.params.chroma || (plane_ok_unaligned(p.pred_u, p.stride_c, p.width >> 1) && plane_ok_unaligned(p.pred_v, p.stride_c, p.width >> 1));
}
// The records of kvz_hip_inter_recon_frames, all checked before anything is launched, then the pass over the destinations.  named[r]:
// a record names pool picture r; first_wg[i]: the workgroups in front of record i, four 16 x 16 tiles each; groups: all of them.
// -> the reason, with *at the record that is refused, or nullptr
inline const char *recon_records_why(const kvz_hip_recon_picture *pictures, int n, const kvz_hip_ref_picture *pool, int n_pool, bool *named, int *first_wg,
                                     unsigned long long &groups, int *at)
{
  for (int &i = *at = 0; i < n; ++i) {
    const kvz_hip_recon_picture &p = pictures[i];
    if (!recon_arrays_ok(p)) return "pred_y or cus is null, or cus misaligned";
    if (!recon_luma_ok(p)) return "width / height must be multiples of 8, stride_y >= the width";
    if (!recon_n_refs_ok(p)) return "n_refs outside 1..16";
    if (!recon_chroma_ok(p)) return "a chroma plane is null, or stride_c below half the width";
    for (int r = 0; r < p.params.n_refs; ++r) {
      if (p.refs[r] >= n_pool) return "a reference index outside the pool";
      if (!ref_ok(pool[p.refs[r]], p.params.chroma, p.width, p.height)) return "a named pool picture of another size, with a missing plane or a short stride";
      named[p.refs[r]] = true;
    }
    for (int j = 0; j < i; ++j)
      if (p.pred_y == pictures[j].pred_y) return "pred_y shared with another picture";
    first_wg[i] = (int)groups;
    groups += ((unsigned long long)((p.width + 15) >> 4) * (unsigned long long)((p.height + 15) >> 4) + 3) / 4;
    if (groups > 0x7fffffffull) return "the pictures of the call exceed the grid";
  }
  // no destination may be a plane of a pool picture that some record names
  for (int &i = *at = 0; i < n; ++i)
    for (int r = 0; r < n_pool; ++r)
      if (const kvz_hip_recon_picture &p = pictures[i]; named[r] && (p.pred_y == pool[r].y || (p.params.chroma && (p.pred_u == pool[r].u || p.pred_v == pool[r].v))))
        return "a destination plane is a named pool plane";
  return nullptr;
}

}  // namespace

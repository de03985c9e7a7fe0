// chain_host.h -- the host side that the multi-picture entries of the picture chain share (kvz_hip_*_frames, kvz_hip_*_frames_ts and the
// filter stages' kvz_hip_cu_qp_frames, kvz_hip_deblock_frames, kvz_hip_sao_stats_frames, kvz_hip_sao_frames, kvz_hip_inter_recon_frames):
// the refusal that names a record, the prologue on the record count, what every residual-stage entry requires of one picture's
// arguments and of each option (the single-picture entries pack their arguments into a record and ask the same checks), the checks of
// a kvz_hip_chain_picture / kvz_hip_chain_picture_ts record, the tile grid on the host with the pool of
// boundaries that the grids of a call share, and the record checks of the hash stage (kvz_hip_picture_hash_frame(s),
// kvz_hip_array_checksum_batch; tests/test_picture_hash_abi.py runs those without a device).
//
// Host only: pointer and integer arithmetic on the structs of kvz_hip.h, which compare pointers and never follow them (a
// kvz_hip_tile_grid and a kvz_hip_trskip are host memory and are read).  No device code and no HIP call, so a plain C++17 compiler
// takes this header with kvz_hip.h alone (tests/test_chain_host_checks.py runs the record checks that way, without a device).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/kvz_hip.h"

namespace kvzhip {
void set_error_msg(const char *what);           // api.hip
}

namespace {

// ---- refusing record i of a call ----
inline int refuse_picture(const char *entry, int i, const char *why)
{
  char msg[200];
  snprintf(msg, sizeof msg, "%s: invalid argument in picture %d (%s)", entry, i, why);
  kvzhip::set_error_msg(msg);
  return KVZ_HIP_ERR_INVALID;
}

// How every multi-picture entry begins: a context, no pictures is a no-op, and the count in range (KVZ_CHECK_CTX, kvz_hip_internal.h)
#define KVZ_CHAIN_PROLOGUE(pictures, n_pictures)                                                                               \
  KVZ_CHECK_CTX();                                                                                                             \
  if ((n_pictures) == 0) return KVZ_HIP_OK;                                                                                    \
  if (!(pictures) || (n_pictures) < 0 || (n_pictures) > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__)

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
  if (width < 8 || height < 8 || ((width | height) & 7) || width > 16384 || height > 16384 || p.stride_y < (uint32_t)width ||
      p.src.stride_y < (uint32_t)width || (p.params.scaling_list != 0) != lists)
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

// ---- the hash stage: kvz_hip_picture_hash_frame(s) and kvz_hip_array_checksum_batch ----
static_assert(sizeof(kvz_hip_lcu_hash) == 24 && sizeof(kvz_hip_picture_hash) == 40 && sizeof(kvz_hip_hash_picture) == 104 &&
              sizeof(kvz_hip_hash_plane) == 24, "layout documented in kvz_hip.h");

// the plane rule of the whole-picture SAO entries: 4-byte aligned base and stride, stride >= the width
inline bool hash_plane_ok(const void *p, uint32_t stride, int w)
{
  return p && !((uintptr_t)p & 3) && !(stride & 3) && stride >= (uint32_t)w;
}

// kvz_hip_picture_hash_frames, and kvz_hip_picture_hash_frame with its arguments as record 0
inline const char *hash_record_why(const kvz_hip_hash_picture *pictures, int i)
{
  const kvz_hip_hash_picture &p = pictures[i];
  const int width = p.width, height = p.height;
  if (!p.lcu_out || !p.out || ((uintptr_t)p.lcu_out & 3) || ((uintptr_t)p.out & 7)) return "lcu_out or out is null or misaligned";
  if (width < 8 || height < 8 || ((width | height) & 7) || width > 16384 || height > 16384 || !hash_plane_ok(p.rec_y, p.stride_y, width))
    return "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8";
  if (p.chroma && (!hash_plane_ok(p.rec_u, p.stride_c, width >> 1) || !hash_plane_ok(p.rec_v, p.stride_c, width >> 1)))
    return "a chroma plane is null or misaligned, or its stride is";
  if (p.src.y) {
    if (p.src.width != width || p.src.height != height) return "src.width / src.height differ from width / height";
    if (!hash_plane_ok(p.src.y, p.src.stride_y, width) ||
        (p.chroma && (!hash_plane_ok(p.src.u, p.src.stride_c, width >> 1) || !hash_plane_ok(p.src.v, p.src.stride_c, width >> 1))))
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

}  // namespace

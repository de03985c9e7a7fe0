// intra_recon_multi_ts.hip -- kvz_hip_intra_recon_frames_ts: kvz_hip_intra_recon_frame_ts (intra_recon_ts.hip) for up to sixteen
// pictures that do not depend on each other, in one call.  Tiles fill a launch from inside a picture (intra_recon_tiles.hip), several
// pictures fill it from the side (intra_recon_multi.hip); here they combine: launch t holds wave t of every tile of every picture, and
// the call makes as many dependent launches as the largest tile of any picture alone.
//
// The kernels are the four instantiations of intra_recon_core.h whose argument is the table of per-picture records with the shared
// pool of tile boundaries (intra_batch_ts<SL, TS>): flat lists or tables, with or without the two trials of transform skip.  SL and
// TS are template parameters of intra_tu, so a call is homogeneous in them and the table's type says which kernel runs; a picture
// without a grid is one tile.  They have this translation unit to themselves, so that the other kernels are compiled as they always
// were.  A workgroup reads its picture's record and its tile's boundaries from the kernel arguments with scalar loads and derives its
// LCU's constants with flat_consts / sl_consts and its LCU's bit cost as the single-picture kernels do, hence the same bytes.
#include "intra_recon_core.h"

static_assert(sizeof(kvz_hip_chain_picture_ts) == 200 && sizeof(kvz_hip_trskip) == 16 && KVZ_HIP_CHAIN_TILE_BOUNDS >= 256 &&
              KVZ_HIP_CHAIN_TILE_BOUNDS % 2 == 0 && KVZ_HIP_CHAIN_TILE_BOUNDS <= 65536, "layouts documented in kvz_hip.h");

namespace {

// intra_recon_init_kernel for every picture that has cbf_out or costs: grid (blocks of the largest such picture, pictures)
__global__ __launch_bounds__(256) void intra_recon_init_multi_ts_kernel(intra_batch_ts_data b)
{
  const intra_pic_ts &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  const int sy = i / a.cus_stride, sx = i - sy * a.cus_stride;
  int cu_x, cu_y, leaf;
  if (!intra_cu_of(a.cus[(size_t)i * 5], 4 * sx, 4 * sy, a.width, a.height, cu_x, cu_y, leaf)) return;
  if (a.cbf_out) a.cbf_out[i] = 0;
  if (a.cost && cu_x == 4 * sx && cu_y == 4 * sy) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a.cost[(size_t)i * 6 + j] = 0u;
  }
}

int refuse(const char *entry, int i, const char *why)
{
  char msg[200];
  snprintf(msg, sizeof msg, "%s: invalid argument in picture %d (%s)", entry, i, why);
  kvzhip::set_error_msg(msg);
  return KVZ_HIP_ERR_INVALID;
}

template <bool SL, bool TS>
int launch_waves(const intra_batch_ts_data &d, int waves, dim3 grid, hipStream_t st)
{
  intra_batch_ts<SL, TS> b;
  static_cast<intra_batch_ts_data &>(b) = d;
  for (int t = 0; t < waves; ++t) {
    hipLaunchKernelGGL((intra_recon_wave_kernel<intra_batch_ts<SL, TS>>), grid, dim3(WG), 0, st, b, t);
    KVZ_CHECK_LAUNCH("intra_recon_wave_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_intra_recon_frames_ts(const kvz_hip_chain_picture_ts *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (n_pictures == 0) return KVZ_HIP_OK;
  if (!pictures || n_pictures < 0 || n_pictures > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__);
  bool options = false;
  for (int i = 0; i < n_pictures; ++i)
    options = options || pictures[i].grid || pictures[i].tables.quant || pictures[i].tables.dequant || pictures[i].ts;
  if (!options) {
    // no options at all: the entry without them on the embedded records, launching that entry's kernel
    kvz_hip_chain_picture plain[KVZ_HIP_MAX_CHAIN_PICTURES];
    for (int i = 0; i < n_pictures; ++i) plain[i] = pictures[i].pic;
    return kvz_hip_intra_recon_frames(plain, n_pictures, s);
  }
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant, skip = pictures[0].ts != nullptr;
  intra_batch_ts_data b;
  __builtin_memset(&b, 0, sizeof b);
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  int waves = 0, groups = 0, planes = 1, init_scus = 0, used = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_ts &r = pictures[i];
    const kvz_hip_chain_picture &p = r.pic;
    const bool has_lists = r.tables.quant || r.tables.dequant;
    if (has_lists != lists || (r.ts != nullptr) != skip)
      return refuse(__func__, i, "a call is homogeneous: every record carries tables or none does, every record carries ts or none does");
    if (has_lists && (!r.tables.quant || !r.tables.dequant || (((uintptr_t)r.tables.quant | (uintptr_t)r.tables.dequant) & 15)))
      return refuse(__func__, i, "a table is null or not 16-byte aligned");
    if (!intra_frame_args_ok(&p.src, p.rec_y, p.stride_y, p.rec_u, p.rec_v, p.stride_c, p.cus, p.intra_modes, p.coeff_y, p.coeff_u, p.coeff_v, p.costs,
                             &p.params, has_lists))
      return refuse(__func__, i, "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given");
    if (r.ts && (!r.tr_skip_out || (!r.ts->lcu_bit_cost && r.ts->bit_cost < 0) || ((uintptr_t)r.ts->lcu_bit_cost & 3)))
      return refuse(__func__, i, "ts without tr_skip_out, a negative bit_cost without lcu_bit_cost, or a misaligned lcu_bit_cost");
    // one QP for the picture: what the one-QP entry refuses
    if (!p.lcu_qp && p.params.qp < 0) return refuse(__func__, i, "a negative qp without lcu_qp");
    kvz_hip_tile_grid g;
    if (!tile_grid_make(r.grid, p.src.width, p.src.height, &g)) return refuse(__func__, i, "invalid tile grid");
    if (r.grid && used + g.cols + g.rows + 2 > KVZ_HIP_CHAIN_TILE_BOUNDS)
      return refuse(__func__, i, "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record");
    for (int j = 0; j < i; ++j) {
      const kvz_hip_chain_picture &o = pictures[j].pic;
      if (p.rec_y == o.rec_y || p.cus == o.cus || p.coeff_y == o.coeff_y || (r.ts && r.tr_skip_out == pictures[j].tr_skip_out))
        return refuse(__func__, i, "an output shared with another picture");
    }
    const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
    intra_pic_ts &a = b.p[i];
    a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
    a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
    a.src_stride[0] = p.src.stride_y; a.src_stride[1] = a.src_stride[2] = p.src.stride_c;
    a.rec_stride[0] = p.stride_y; a.rec_stride[1] = a.rec_stride[2] = p.stride_c;
    a.coeff[0] = p.coeff_y; a.coeff[1] = chroma ? p.coeff_u : nullptr; a.coeff[2] = chroma ? p.coeff_v : nullptr;
    a.cus = (u32 *)p.cus; a.modes = p.intra_modes; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
    a.qp = clip_lcu_qp(p.params.qp);                                          // the single-picture tiled kernels clamp the picture's QP too
    a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
    a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
    if (has_lists) { a.quant = r.tables.quant; a.dequant = r.tables.dequant; }
    if (r.ts) { a.lcu_bit_cost = r.ts->lcu_bit_cost; a.tr_skip_out = r.tr_skip_out; a.bit_cost = r.ts->bit_cost; }
    if (r.grid) {
      // the boundaries the call uses, 16 bits each (an LCU index is at most 256): cols + 1 of the columns, then rows + 1 of the rows
      a.cols = (u8)g.cols; a.rows = (u8)g.rows;
      a.col_at = (uint16_t)used;
      for (int j = 0; j <= g.cols; ++j) bounds[used++] = (uint16_t)g.col_bd[j];
      a.row_at = (uint16_t)used;
      for (int j = 0; j <= g.rows; ++j) bounds[used++] = (uint16_t)g.row_bd[j];
    }
    const int lcus_y = (height + 63) >> 6;
    waves = max(waves, tile_grid_waves(g));
    groups = max(groups, lcus_y * g.cols);
    if (chroma) planes = 3;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (width >> 2) * (height >> 2));
  }
  for (int j = 0; j < used; ++j) b.bd[j >> 1] |= (u32)bounds[j] << (16 * (j & 1));
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags, the grids and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(intra_recon_init_multi_ts_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("intra_recon_init_multi_ts_kernel");
  }
  const dim3 grid((unsigned)groups, (unsigned)planes, (unsigned)n_pictures);
  if (lists) return skip ? launch_waves<true, true>(b, waves, grid, st) : launch_waves<true, false>(b, waves, grid, st);
  return skip ? launch_waves<false, true>(b, waves, grid, st) : launch_waves<false, false>(b, waves, grid, st);
}

}  // extern "C"

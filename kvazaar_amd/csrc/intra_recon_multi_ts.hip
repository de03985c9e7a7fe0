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
  zero_cu_outputs(a, i, intra_cu_rule());
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
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
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
    // the record's own checks, its grid and the grid's place in the pool, then the outputs of the earlier records: the order decides
    // which reason a record with two defects reports
    const char *why = chain_record_ts_why(pictures, i, true, lists, skip);
    kvz_hip_tile_grid g;
    pic_tiles t;
    if (!why && !tile_grid_make(r.grid, p.src.width, p.src.height, &g)) why = "invalid tile grid";
    if (!why && !tile_pool_add(r.grid, g, bounds, used, &t)) why = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record";
    if (!why) why = chain_record_ts_shared(pictures, i);
    if (why) return refuse_picture(__func__, i, why);
    intra_pic_ts &a = b.p[i];
    fill(a, p, clip_lcu_qp(p.params.qp));                                     // the single-picture tiled kernels clamp the picture's QP too
    if (lists) { a.quant = r.tables.quant; a.dequant = r.tables.dequant; }
    if (r.ts) { a.lcu_bit_cost = r.ts->lcu_bit_cost; a.tr_skip_out = r.tr_skip_out; a.bit_cost = r.ts->bit_cost; }
    // the kernel reads cols == 0 as "no grid": a picture without one keeps the zeros, where pic_tiles says one tile
    if (r.grid) { a.cols = t.cols; a.rows = t.rows; a.col_at = t.col_at; a.row_at = t.row_at; }
    waves = max(waves, tile_grid_waves(g));
    groups = max(groups, (int)t.lcus_y * g.cols);
    if (a.chroma) planes = 3;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (a.width >> 2) * (a.height >> 2));
  }
  tile_pool_pack(bounds, used, b.bd);
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

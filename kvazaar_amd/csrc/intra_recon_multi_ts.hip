// intra_recon_multi_ts.hip -- kvz_hip_intra_recon_frames_ts: kvz_hip_intra_recon_frame_ts (intra_recon_ts.hip) for up to sixteen
// pictures that do not depend on each other, in one call.  Tiles fill a launch from inside a picture (intra_recon_tiles.hip), several
// pictures fill it from the side (intra_recon_multi.hip); here they combine: launch t holds wave t of every tile of every picture, and
// the call makes as many dependent launches as the largest tile of any picture alone.
//
// The kernels are the four instantiations of intra_recon_core.h whose argument is the table of per-picture records with the shared
// pool of tile boundaries (intra_batch_ts<SL, TS>): flat lists or tables, with or without the two trials of transform skip; behind
// them init_pictures_kernel (frame_sources.h) on the same table.  SL and TS are template parameters of intra_tu, so a call is
// homogeneous in them and the table's type says which kernel runs; a picture without a grid is one tile.  They have this translation
// unit to themselves, so that the other kernels are compiled as they always were.  A workgroup reads its picture's record and its
// tile's boundaries from the kernel arguments with scalar loads and derives its LCU's constants with flat_consts / sl_consts and its
// LCU's bit cost as the single-picture kernels do, hence the same bytes.  The records are checked, the pool filled and the launches
// sized by the walk that the six multi-picture entries of the residual stages share (chain_records_why, chain_host.h).
#include "intra_recon_core.h"

static_assert(sizeof(kvz_hip_chain_picture_ts) == 200 && sizeof(kvz_hip_trskip) == 16 && KVZ_HIP_CHAIN_TILE_BOUNDS >= 256 &&
              KVZ_HIP_CHAIN_TILE_BOUNDS % 2 == 0 && KVZ_HIP_CHAIN_TILE_BOUNDS <= 65536, "layouts documented in kvz_hip.h");

namespace {

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
  chain_tiles tiles;
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, true, &tiles, &plan, &at)) return refuse_picture(__func__, at, why);
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant, skip = pictures[0].ts != nullptr;
  intra_batch_ts_data b;
  __builtin_memset(&b, 0, sizeof b);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_ts &r = pictures[i];
    fill(b.p[i], r.pic, clip_lcu_qp(r.pic.params.qp));                          // the single-picture tiled kernels clamp the picture's QP too
    fill_lists(b.p[i], r.tables);
    fill_trskip(b.p[i], r.ts, r.tr_skip_out);
    fill_tiles(b.p[i], r.grid, tiles.pic[i]);
  }
  tile_pool_pack(tiles.bounds, tiles.used, b.bd);
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags, the grids and the presence of cbf_out / costs alone
  if (int e = init_pictures<intra_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  const dim3 grid((unsigned)plan.groups, (unsigned)plan.planes, (unsigned)n_pictures);
  if (lists) return skip ? launch_waves<true, true>(b, plan.waves, grid, st) : launch_waves<true, false>(b, plan.waves, grid, st);
  return skip ? launch_waves<false, true>(b, plan.waves, grid, st) : launch_waves<false, false>(b, plan.waves, grid, st);
}

}  // extern "C"

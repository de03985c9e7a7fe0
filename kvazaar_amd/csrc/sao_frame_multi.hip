// sao_frame_multi.hip -- kvz_hip_sao_stats_frames and kvz_hip_sao_frames: kvz_hip_sao_stats_frame (sao_frame.hip) and
// kvz_hip_sao_frame_tiles (sao_frame_tiles.hip) for up to sixteen pictures that do not depend on each other, in one call and one launch
// each, the picture being the grid's second dimension.  Both stages are one short launch per picture, so what a host with P pictures
// gains is the launches it no longer repeats.
//
// The kernels are the instantiations of sao_stats_core.h and sao_frame_core.h whose trailing argument is the table of per-picture
// records -- a record is the single entry's kernel argument -- for the reconstruction with the shared pool of tile boundaries; they
// have this translation unit to themselves, so that the single-picture kernels are compiled as they always were.  A workgroup reads
// its picture's record from the kernel arguments with scalar loads.  A launch is sized for the largest picture; the surplus
// workgroups of a smaller one leave at once.
#include "sao_stats_core.h"

static_assert(sizeof(kvz_hip_filter_picture) == 264, "layout documented in kvz_hip.h");

extern "C" {

int kvz_hip_sao_stats_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  stats_batch b;
  __builtin_memset(&b, 0, sizeof b);
  int groups = 0, none = 0, at = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = filter_records_why(pictures, n_pictures, sao_stats_record_why, sao_stats_output_shared, nullptr, none, nullptr, &at))
    return refuse_picture(__func__, at, why);
  for (int i = 0; i < n_pictures; ++i) {
    stats_args &a = b.p[i];
    sao_stats_fill(a, pictures[i]);
    groups = max(groups, a.n_lcu * (pictures[i].chroma ? 3 : 1));
  }
  // the launch depends on the sizes and the chroma flags alone (cands is a branch at the end of a workgroup): grid (plane-LCUs of the
  // largest picture, pictures); the kernel's own arguments are not read
  hipLaunchKernelGGL(sao_stats_frame_kernel<stats_batch>, dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, ctx_stream(s), b.p[0], b);
  KVZ_CHECK_LAUNCH("sao_stats_frame_kernel<pictures>");
  return KVZ_HIP_OK;
}

int kvz_hip_sao_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  frame_batch b;
  __builtin_memset(&b, 0, sizeof b);
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  pic_tiles tiles[KVZ_HIP_MAX_CHAIN_PICTURES];
  int used = 0, groups = 0, at = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = filter_records_why(pictures, n_pictures, sao_record_why, sao_output_shared, bounds, used, tiles, &at))
    return refuse_picture(__func__, at, why);
  for (int i = 0; i < n_pictures; ++i) {
    frame_pic &r = b.p[i];
    r.tiles = tiles[i];
    sao_frame_fill(r.a, pictures[i]);
    groups = max(groups, r.a.tiles_y + 2 * r.a.tiles_c);
  }
  tile_pool_pack(bounds, used, b.pool.bd);
  // the launch depends on the sizes and the chroma flags alone: grid (tiles of the largest picture, pictures); the kernel's own
  // arguments are not read
  hipLaunchKernelGGL(sao_frame_kernel<frame_batch>, dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, ctx_stream(s), b.p[0].a, b);
  KVZ_CHECK_LAUNCH("sao_frame_kernel<pictures>");
  return KVZ_HIP_OK;
}

}  // extern "C"

// deblock_multi.hip -- kvz_hip_deblock_frames: kvz_hip_deblock_frame_tiles (deblock_tiles.hip) for up to sixteen pictures that do not
// depend on each other, in one call: that entry's two launches, all vertical edges and then all horizontal edges, each covering all
// pictures, the picture being the grid's second dimension.  The stage is bound by its launches, so what a host with P pictures gains
// is the launches it no longer repeats.
//
// The kernels are the instantiations of deblock_core.h whose trailing argument is the table of per-picture records with the shared
// pool of tile boundaries (deblock_batch); they have this translation unit to themselves, so that the single-picture kernels are
// compiled as they always were.  A workgroup reads its picture's record, deblock parameters included, from the kernel arguments
// with scalar loads.  A launch is sized for the largest picture; the surplus workgroups of a smaller one leave at once.
#include "deblock_core.h"

static_assert(sizeof(kvz_hip_filter_picture) == 264, "layout documented in kvz_hip.h");

extern "C" int kvz_hip_deblock_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  deblock_batch b;
  __builtin_memset(&b, 0, sizeof b);
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  pic_tiles tiles[KVZ_HIP_MAX_CHAIN_PICTURES];
  int used = 0, at = 0;
  size_t threads = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = filter_records_why(pictures, n_pictures, deblock_record_why, deblock_output_shared, bounds, used, tiles, &at))
    return refuse_picture(__func__, at, why);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_filter_picture &p = pictures[i];
    deblock_pic &r = b.p[i];
    r.tiles = tiles[i];
    r.cus = (const u32 *)p.cus;
    r.rec_y = p.rec_y; r.rec_u = p.chroma ? p.rec_u : nullptr; r.rec_v = p.chroma ? p.rec_v : nullptr;
    r.stride_y = p.stride_y; r.stride_c = p.stride_c;
    r.prm = p.deblock;
    r.width = (uint16_t)p.width; r.height = (uint16_t)p.height;
    const size_t t = (size_t)(p.width >> 3) * (size_t)(p.height >> 3) * 2;
    threads = t > threads ? t : threads;
  }
  tile_pool_pack(bounds, used, b.pool.bd);
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes alone: grid (blocks of the largest picture, pictures)
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n_pictures);
  const frame_t none = {};                                                    // not read: every thread takes its picture's record
  hipLaunchKernelGGL((deblock_pass_kernel<0, deblock_batch>), grid, dim3(256), 0, st, (u8 *)nullptr, 0u, (u8 *)nullptr, (u8 *)nullptr, 0u, none,
                     pictures[0].deblock, b);
  KVZ_CHECK_LAUNCH("deblock_pass_kernel<vertical edges, pictures>");
  hipLaunchKernelGGL((deblock_pass_kernel<1, deblock_batch>), grid, dim3(256), 0, st, (u8 *)nullptr, 0u, (u8 *)nullptr, (u8 *)nullptr, 0u, none,
                     pictures[0].deblock, b);
  KVZ_CHECK_LAUNCH("deblock_pass_kernel<horizontal edges, pictures>");
  return KVZ_HIP_OK;
}

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
  int groups = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_filter_picture &p = pictures[i];
    const int width = p.width, height = p.height, chroma = p.chroma ? 1 : 0;
    if (p.deblock.chroma != p.chroma) return refuse_picture(__func__, i, "deblock.chroma differs from chroma");
    if (p.src.width != width || p.src.height != height) return refuse_picture(__func__, i, "src.width / src.height differ from width / height");
    if (!p.stats || ((uintptr_t)p.stats & 3) || ((uintptr_t)p.cands & 3)) return refuse_picture(__func__, i, "stats is null, or stats or cands misaligned");
    if (!picture_ok(width, height) || !plane_ok(p.src.y, p.src.stride_y, width) || !plane_ok(p.rec_y, p.stride_y, width))
      return refuse_picture(__func__, i, "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8");
    if (chroma && (!plane_ok(p.src.u, p.src.stride_c, width >> 1) || !plane_ok(p.src.v, p.src.stride_c, width >> 1) ||
                   !plane_ok(p.rec_u, p.stride_c, width >> 1) || !plane_ok(p.rec_v, p.stride_c, width >> 1)))
      return refuse_picture(__func__, i, "a chroma plane is null or misaligned, or its stride is");
    for (int j = 0; j < i; ++j)
      if (p.stats == pictures[j].stats || (p.cands && p.cands == pictures[j].cands)) return refuse_picture(__func__, i, "an output shared with another picture");
    stats_args &a = b.p[i];
    a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
    a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
    a.src_stride[0] = p.src.stride_y; a.src_stride[1] = p.src.stride_c;
    a.rec_stride[0] = p.stride_y; a.rec_stride[1] = p.stride_c;
    a.width = width; a.height = height;
    a.lcus_x = (width + 63) >> 6;
    a.n_lcu = a.lcus_x * ((height + 63) >> 6);
    a.stats = (int *)p.stats; a.cands = (int *)p.cands;
    groups = max(groups, a.n_lcu * (chroma ? 3 : 1));
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
  int used = 0, groups = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_filter_picture &p = pictures[i];
    const int width = p.width, height = p.height, chroma = p.chroma ? 1 : 0;
    if (p.deblock.chroma != p.chroma) return refuse_picture(__func__, i, "deblock.chroma differs from chroma");
    if (!p.sao_luma || ((uintptr_t)p.sao_luma & 3) || p.dst_y == p.rec_y) return refuse_picture(__func__, i, "sao_luma is null or misaligned, or dst_y is rec_y");
    if (!picture_ok(width, height) || !plane_ok(p.rec_y, p.stride_y, width) || !plane_ok(p.dst_y, p.dst_stride_y, width))
      return refuse_picture(__func__, i, "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8");
    if (chroma && (!p.sao_chroma || ((uintptr_t)p.sao_chroma & 3) || p.dst_u == p.rec_u || p.dst_v == p.rec_v ||
                   !plane_ok(p.rec_u, p.stride_c, width >> 1) || !plane_ok(p.rec_v, p.stride_c, width >> 1) ||
                   !plane_ok(p.dst_u, p.dst_stride_c, width >> 1) || !plane_ok(p.dst_v, p.dst_stride_c, width >> 1)))
      return refuse_picture(__func__, i, "sao_chroma or a chroma plane is null or misaligned, a chroma stride is, or a dst plane is its rec plane");
    kvz_hip_tile_grid g;
    if (!tile_grid_make(p.grid, width, height, &g)) return refuse_picture(__func__, i, "invalid tile grid");
    frame_pic &r = b.p[i];
    if (!tile_pool_add(p.grid, g, bounds, used, &r.tiles))
      return refuse_picture(__func__, i, "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record");
    for (int j = 0; j < i; ++j)
      if (p.dst_y == pictures[j].dst_y) return refuse_picture(__func__, i, "an output shared with another picture");
    frame_args &a = r.a;
    a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
    a.dst[0] = p.dst_y; a.dst[1] = chroma ? p.dst_u : nullptr; a.dst[2] = chroma ? p.dst_v : nullptr;
    a.rec_stride[0] = p.stride_y; a.rec_stride[1] = p.stride_c;
    a.dst_stride[0] = p.dst_stride_y; a.dst_stride[1] = p.dst_stride_c;
    a.width = width; a.height = height;
    a.lcus_x = (width + 63) >> 6;
    a.tiles_y = a.lcus_x * ((height + 15) >> 4);
    a.tiles_c = chroma ? a.lcus_x * ((height + 63) >> 6) : 0;
    a.sao[0] = p.sao_luma; a.sao[1] = chroma ? p.sao_chroma : nullptr;
    groups = max(groups, a.tiles_y + 2 * a.tiles_c);
  }
  tile_pool_pack(bounds, used, b.pool.bd);
  // the launch depends on the sizes and the chroma flags alone: grid (tiles of the largest picture, pictures); the kernel's own
  // arguments are not read
  hipLaunchKernelGGL(sao_frame_kernel<frame_batch>, dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, ctx_stream(s), b.p[0].a, b);
  KVZ_CHECK_LAUNCH("sao_frame_kernel<pictures>");
  return KVZ_HIP_OK;
}

}  // extern "C"

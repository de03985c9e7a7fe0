// sao_frame_tiles.hip -- kvz_hip_sao_frame_tiles: the SAO reconstruction (sao_frame.hip) of a picture cut into tiles.  The reference
// reconstructs every tile as a picture of its own (kvz_sao_reconstruct takes its bounds from state->tile->frame, sao.c:278-337), so
// an edge-offset pixel whose neighbour a or b lies in another tile keeps its deblocked value; band offset and copy do not look at
// neighbours.  The kernel is the instantiation of sao_frame_core.h that takes the grid; it has this translation unit to itself.
#include "sao_frame_core.h"

extern "C" int kvz_hip_sao_frame_tiles(const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v,
                                       uint32_t stride_c, kvz_hip_pixel *dst_y, uint32_t dst_stride_y, kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v,
                                       uint32_t dst_stride_c, int width, int height, const kvz_hip_sao_info *sao_luma,
                                       const kvz_hip_sao_info *sao_chroma, int chroma, const kvz_hip_tile_grid *grid, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  kvz_hip_tile_grid g;
  sao_pack(&p, rec_y, stride_y, rec_u, rec_v, stride_c, dst_y, dst_stride_y, dst_u, dst_v, dst_stride_c, width, height, sao_luma, sao_chroma, chroma, grid);
  if (!picture_ok(width, height) || !tile_grid_make(grid, width, height, &g)) return kvzhip::invalid_arg(__func__);
  return sao_frame_launch(__func__, p, s, g);
}

// deblock_tiles.hip -- kvz_hip_deblock_frame_tiles: the deblocking filter (deblock.hip) over a picture cut into tiles.  The reference
// filters every tile as a picture of its own (filter.c:690-779 take all bounds from state->tile->frame, and
// loop_filter_across_tiles_enabled_flag is 0), so the edges that lie on a boundary between tiles stay as they are.  An unfiltered
// boundary decouples its two sides -- no filtered pixel depends on a pixel beyond it -- so the two passes over the whole picture, all
// vertical edges and then all horizontal edges, remain the reference's order inside every tile.  The kernels are the instantiations
// of deblock_core.h that take the grid; they have this translation unit to themselves.
#include "deblock_core.h"

extern "C" int kvz_hip_deblock_frame_tiles(kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c,
                                           int width, int height, const kvz_hip_cu_info *cus, const kvz_hip_tile_grid *grid,
                                           const kvz_hip_deblock_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  if (const int rc = deblock_refusal(__func__, deblock_pack(&p, rec_y, stride_y, rec_u, rec_v, stride_c, width, height, cus, grid, params) ? &p : nullptr)) return rc;
  kvz_hip_tile_grid g;
  if (!tile_grid_make(grid, width, height, &g)) return kvzhip::invalid_arg(__func__);
  return deblock_launch(p, s, g);
}

// cu_qp_tiles.hip -- kvz_hip_cu_qp_frame_tiles: the QP map (cu_qp.hip) of a picture cut into tiles.  A tile is a leaf state of the
// reference, so last_qp starts again from the picture's QP in every tile (encoderstate.c:729), and with WPP inside tiles in every LCU
// row of every tile.  What an LCU does with `last` does not depend on tiles: launches 1 and 3 are those of cu_qp.hip; the scan
// between them runs over the chains of the grid -- a workgroup per tile (the tile's LCUs in raster order inside the tile), or per
// LCU row and tile column -- and finds a chain's LCUs in the array, which stays in picture raster order (cu_qp_core.h).
#include "cu_qp_core.h"

namespace {

static_assert(sizeof(kvz_hip_cu_qp_tiles_params) == 8, "layout documented in kvz_hip.h");

}  // namespace

extern "C" {

int kvz_hip_cu_qp_frame_tiles(kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp, int8_t *lcu_last_qp,
                              const kvz_hip_tile_grid *grid, const kvz_hip_cu_qp_tiles_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_filter_picture p;
  kvz_hip_tile_grid g;
  if (!cu_qp_pack(&p, cus, cbf, width, height, lcu_qp, lcu_last_qp, grid, params) || !cu_qp_arrays_ok(p) || !picture_ok(width, height) ||
      !cu_qp_chains_ok(p) || !tile_grid_make(grid, width, height, &g))
    return kvzhip::invalid_arg(__func__);
  // the launch sequence depends on width, height, the grid and chain_rows alone
  const int lcus_x = (width + 63) >> 6, lcus_y = (height + 63) >> 6;
  const tile_chains chains = { g, lcus_x, params->chain_rows };
  return cu_qp_launch(p, s, dim3((unsigned)g.cols, (unsigned)(params->chain_rows ? lcus_y : g.rows)), 0, 0, chains);
}

}  // extern "C"

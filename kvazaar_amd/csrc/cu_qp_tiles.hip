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
  if (!cus || !cbf || !lcu_qp || !lcu_last_qp || !params || ((uintptr_t)cus & 3)) return kvzhip::invalid_arg(__func__);
  if (width < 8 || height < 8 || ((width | height) & 7) || width > 16384 || height > 16384) return kvzhip::invalid_arg(__func__);
  if (params->start_qp < 0 || params->start_qp > 51 || (params->chain_rows != 0 && params->chain_rows != 1)) return kvzhip::invalid_arg(__func__);
  kvz_hip_tile_grid g;
  if (!tile_grid_make(grid, width, height, &g)) return kvzhip::invalid_arg(__func__);
  const int lcus_x = (width + 63) >> 6, lcus_y = (height + 63) >> 6;
  cu_qp_args a;
  a.cus = (u32 *)cus; a.cbf = cbf; a.lcu_qp = lcu_qp; a.lcu_last_qp = lcu_last_qp;
  a.cus_stride = width >> 2; a.lcus_x = lcus_x;
  a.width = width; a.height = height;
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on width, height, the grid and chain_rows alone
  hipLaunchKernelGGL(cu_qp_first_kernel, dim3((unsigned)lcus_x, (unsigned)lcus_y), dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_first_kernel");
  const tile_chains chains = { g, lcus_x, params->chain_rows };
  hipLaunchKernelGGL(cu_qp_chain_kernel<tile_chains>, dim3((unsigned)g.cols, (unsigned)(params->chain_rows ? lcus_y : g.rows)), dim3(256), 0, st,
                     lcu_last_qp, 0, 0, params->start_qp, chains);
  KVZ_CHECK_LAUNCH("cu_qp_chain_kernel<tiles>");
  hipLaunchKernelGGL(cu_qp_write_kernel, dim3((unsigned)lcus_x, (unsigned)lcus_y), dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_write_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

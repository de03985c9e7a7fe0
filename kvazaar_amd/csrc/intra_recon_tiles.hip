// intra_recon_tiles.hip -- kvz_hip_intra_recon_frame_tiles: kvz_hip_intra_recon_frame_qp (intra_recon_qp.hip) for a picture cut
// into tiles.  The reference reconstructs intra CUs against state->tile->frame (intra.c:334-588, search.c:761-835): a TU's
// neighbours exist inside its tile only.  The kernel is the instantiation of intra_recon_core.h that takes the grid as a second
// trailing argument; it has this translation unit to itself, so that the two untiled kernels are compiled as they always were.
//
// The tiles of a picture do not depend on each other, so their wavefronts run side by side: launch t holds wave t of every tile,
// counted from the tile's own origin, and the call makes max over tiles of w_t + 2 (h_t - 1) dependent launches instead of the
// picture's lcus_x + 2 (lcus_y - 1).  A workgroup reads no pixel outside its tile -- the reference's result, and what makes the
// concurrent tiles race-free.
#include "intra_recon_core.h"

extern "C" {

int kvz_hip_intra_recon_frame_tiles(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                    kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                    kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                    kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                    const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_chain_picture p;
  tile_source tiles;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed || !tile_source_make(p, grid, &tiles)) return kvzhip::invalid_arg(__func__);
  return intra_frame(__func__, p, s, qp_source_of(p), tiles);
}

}  // extern "C"

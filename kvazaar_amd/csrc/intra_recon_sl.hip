// intra_recon_sl.hip -- kvz_hip_intra_recon_frame_sl: kvz_hip_intra_recon_frame_tiles (intra_recon_tiles.hip) for a picture coded
// with scaling lists (--scaling-list, --cqmfile).  The kernel is the instantiation of intra_recon_core.h that takes the packed tables
// as a third trailing argument; it has this translation unit to itself, so that the three other kernels are compiled as they
// always were.  A workgroup is one LCU of one plane: the table pointers of its four transform sizes follow from the LCU's QP and are
// derived once, before the walk.  The tables are read-only and shared by every workgroup: they stay in the L2, no staging in LDS.
#include "intra_recon_core.h"

extern "C" {

int kvz_hip_intra_recon_frame_sl(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                 kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                 kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                 kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                 const kvz_hip_scaling_tables *tables, const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!tables) {
    // without tables it is the entry without them, launching that entry's kernel; a picture that needs tables is refused here
    if (params && params->scaling_list != 0) return kvzhip::invalid_arg(__func__);
    return kvz_hip_intra_recon_frame_tiles(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                           lcu_qp, grid, params, s);
  }
  kvz_hip_chain_picture p;
  tile_source tiles;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed || !chain_tables_ok(*tables) || !tile_source_make(p, grid, &tiles)) return kvzhip::invalid_arg(__func__);
  const sl_source lists = { tables->quant, tables->dequant };
  return intra_frame(__func__, p, s, qp_source_of(p), tiles, lists);
}

}  // extern "C"

// intra_recon_ts_cabac.hip -- kvz_hip_intra_recon_frame_ts_cabac: kvz_hip_intra_recon_frame_ts (intra_recon_ts.hip) with the reference's
// pricing rule inside the transform-skip decision (kvz_get_coeff_cost, rdo.c:208-222): where the QP of an LCU is at or above
// cfg.fast_residual_cost_limit, each trial of its 4x4 luma TUs is priced with get_coeff_cabac_cost (coeff_cabac_core.h) on the LCU's
// context set, otherwise with the estimate.  The kernels are the instantiations of intra_recon_core.h that take the pricing source
// after the transform-skip source; they have this translation unit to themselves, so that the other kernels are compiled as they
// always were.  The first lane of each trial's quad counts, both at once, so the chain of dependent TUs grows by one count.
#include "intra_recon_core.h"
#include "coeff_cost_host.h"

extern "C" {

int kvz_hip_intra_recon_frame_ts_cabac(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                       kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                       kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                       kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                       const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                       const kvz_hip_coeff_pricing *pricing, const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!pricing) {
    // without it, it is the entry without it, launching that entry's kernel
    return kvz_hip_intra_recon_frame_ts(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp,
                                        grid, tables, ts, tr_skip_out, params, s);
  }
  kvz_hip_chain_picture p;
  tile_source tiles;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (coeff_pricing_why(pricing, ts) || !packed || !chain_trskip_ok(ts, tr_skip_out) || (tables && !chain_tables_ok(*tables)) ||
      !tile_source_make(p, grid, &tiles))
    return kvzhip::invalid_arg(__func__);
  const ts_source skip = { ts->lcu_bit_cost, tr_skip_out, ts->bit_cost };
  const cabac_source price = { pricing->ctx_sets, pricing->lcu_ctx, pricing->n_sets, pricing->fast_limit };
  if (tables) {
    const sl_source lists = { tables->quant, tables->dequant };
    return intra_frame(__func__, p, s, qp_source_of(p), tiles, lists, skip, price);
  }
  return intra_frame(__func__, p, s, qp_source_of(p), tiles, skip, price);
}

}  // extern "C"

// intra_recon_ts.hip -- kvz_hip_intra_recon_frame_ts: kvz_hip_intra_recon_frame_sl (intra_recon_sl.hip) for a picture coded with
// --transform-skip.  The reference codes every 4x4 luma TU twice, transformed (DST) and transform-skipped, and keeps the cheaper
// trial (kvz_quantize_residual_trskip, transform.c:229-276), priced with the estimate of kvz_get_coeff_cost below
// fast_residual_cost_limit (rdo.c:219-220).  The kernels are the instantiations of intra_recon_core.h that take the transform-skip
// source as their last trailing argument, with flat lists or with the packed tables; they have this translation unit to themselves,
// so that the four other kernels are compiled as they always were.  A 4x4 TU used four lanes of its wave: the second trial runs on
// the next four, in the same instructions, and the chain of dependent TUs grows by the decision (intra_tu, intra_recon_core.h).
#include "intra_recon_core.h"

static_assert(sizeof(kvz_hip_trskip) == 16, "layout documented in kvz_hip.h");

extern "C" {

int kvz_hip_intra_recon_frame_ts(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                 kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                 kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                 kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                 const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                 const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!ts) {
    // without it, it is the entry without it, launching that entry's kernel
    return kvz_hip_intra_recon_frame_sl(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp,
                                        grid, tables, params, s);
  }
  kvz_hip_chain_picture p;
  tile_source tiles;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed || !chain_trskip_ok(ts, tr_skip_out) || (tables && !chain_tables_ok(*tables)) || !tile_source_make(p, grid, &tiles))
    return kvzhip::invalid_arg(__func__);
  const ts_source skip = { ts->lcu_bit_cost, tr_skip_out, ts->bit_cost };
  if (tables) {
    const sl_source lists = { tables->quant, tables->dequant };
    return intra_frame(__func__, p, s, qp_source_of(p), tiles, lists, skip);
  }
  return intra_frame(__func__, p, s, qp_source_of(p), tiles, skip);
}

}  // extern "C"

// inter_residual_ts_cabac.hip -- kvz_hip_inter_residual_frame_ts_cabac: kvz_hip_inter_residual_frame_ts (inter_residual_ts.hip) with the
// reference's pricing rule inside the transform-skip decision (kvz_get_coeff_cost, rdo.c:208-222): where the QP of a TU's LCU is at or
// above cfg.fast_residual_cost_limit, each trial is priced with get_coeff_cabac_cost (coeff_cabac_core.h) on the LCU's context set,
// otherwise with the estimate.  Only the N = 4 launch changes: its kernel is the instantiation of inter_residual_core.h that takes
// the pricing source after the transform-skip source.  The instantiations have this translation unit to themselves, so that the
// kernels of the other entries are compiled as they always were.
#include "inter_residual_core.h"
#include "coeff_cost_host.h"

extern "C" {

int kvz_hip_inter_residual_frame_ts_cabac(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                          kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                          kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                          const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts,
                                          uint8_t *tr_skip_out, const kvz_hip_coeff_pricing *pricing,
                                          const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!pricing) {
    // without it, it is the entry without it, launching that entry's kernels
    return kvz_hip_inter_residual_frame_ts(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, tables, ts,
                                           tr_skip_out, params, s);
  }
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (coeff_pricing_why(pricing, ts) || !packed || !chain_trskip_ok(ts, tr_skip_out)) return kvzhip::invalid_arg(__func__);
  const ts_source skip = { ts->lcu_bit_cost, tr_skip_out, ts->bit_cost, p.params.qp };
  const cabac_source price = { pricing->ctx_sets, pricing->lcu_ctx, pricing->n_sets, pricing->fast_limit };
  // without tables, what the _sl entry refuses without them is refused: scaling_list says whether tables are given
  if (tables) return residual_frame<true, true, true>(__func__, p, tables, s, &skip, &price);
  return residual_frame<false, true, true>(__func__, p, nullptr, s, &skip, &price);
}

}  // extern "C"

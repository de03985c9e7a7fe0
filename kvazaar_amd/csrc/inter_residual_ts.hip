// inter_residual_ts.hip -- kvz_hip_inter_residual_frame_ts: kvz_hip_inter_residual_frame_sl (inter_residual_sl.hip) for a picture coded
// with --transform-skip.  The reference codes every 4x4 luma TU twice, transformed and transform-skipped, and keeps the cheaper trial
// (kvz_quantize_residual_trskip, transform.c:229-276); the price of the coefficients is the estimate of kvz_get_coeff_cost below
// fast_residual_cost_limit (rdo.c:219-220), the only branch of it that does not depend on the CABAC state.  Only the N = 4 launch
// changes: its kernel is the instantiation of inter_residual_core.h that takes the transform-skip source as its last trailing
// argument, with flat lists or with the packed tables.  A luma slot runs the second trial in the threads of the first, on the rows
// they already hold in registers, and writes once, after the decision; the launches of the other sizes are those of the _sl entry.
// The instantiations have this translation unit to themselves, so that the kernels of inter_residual.hip and inter_residual_sl.hip
// are compiled as they always were.
#include "inter_residual_core.h"

static_assert(sizeof(kvz_hip_trskip) == 16, "layout documented in kvz_hip.h");

extern "C" {

int kvz_hip_inter_residual_frame_ts(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                    kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                    kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                    const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts,
                                    uint8_t *tr_skip_out, const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!ts) {
    // without it, it is the entry without it, launching that entry's kernels
    return kvz_hip_inter_residual_frame_sl(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, tables,
                                           params, s);
  }
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed || !chain_trskip_ok(ts, tr_skip_out)) return kvzhip::invalid_arg(__func__);
  const ts_source skip = { ts->lcu_bit_cost, tr_skip_out, ts->bit_cost, p.params.qp };
  // without tables, what the _sl entry refuses without them is refused: scaling_list says whether tables are given
  if (tables) return residual_frame<true, true>(__func__, p, tables, s, &skip);
  return residual_frame<false, true>(__func__, p, nullptr, s, &skip);
}

}  // extern "C"

// inter_residual_sl.hip -- kvz_hip_inter_residual_frame_sl: kvz_hip_inter_residual_frame_qp (inter_residual.hip) for a picture coded
// with scaling lists (--scaling-list, --cqmfile).  The kernels are the instantiations of inter_residual_core.h that take the packed
// tables as a second trailing argument: every TU picks its quantisation and dequantisation table from its size, its plane and
// qp % 6 of its own LCU (sl_consts, quant_core.h) and reads its row of each with 16-byte loads.  The tables are read-only and
// shared by every workgroup, 196 KB each: they stay in the L2 and are not staged in LDS.  The instantiations have this translation
// unit to themselves, so that the kernels of inter_residual.hip are compiled as they always were.
#include "inter_residual_core.h"

extern "C" {

int kvz_hip_inter_residual_frame_sl(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                    kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                    kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                    const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables,
                                    const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!tables) {
    // without tables it is the entry without them, launching that entry's kernels; a picture that needs tables is refused here
    if (params && params->scaling_list != 0) return kvzhip::invalid_arg(__func__);
    return kvz_hip_inter_residual_frame_qp(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, params, s);
  }
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  return residual_frame<true>(__func__, p, tables, s);
}

}  // extern "C"

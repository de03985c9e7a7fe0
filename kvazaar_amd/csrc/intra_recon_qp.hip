// intra_recon_qp.hip -- kvz_hip_intra_recon_frame_qp: kvz_hip_intra_recon_frame (intra_recon.hip) for a picture whose QP changes from
// LCU to LCU.  The kernel is the instantiation of intra_recon_core.h that reads its LCU's QP from an array on the device; it has this
// translation unit to itself, so that the one-QP kernel of intra_recon.hip is compiled as it always was.
#include "intra_recon_core.h"

extern "C" {

int kvz_hip_intra_recon_frame_qp(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                 kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                 kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                 kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_inter_residual_params *params,
                                 kvz_hip_stream s)
{
  // without the array it is the old entry, launching the old entry's kernel
  if (!lcu_qp) return kvz_hip_intra_recon_frame(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs, params, s);
  KVZ_CHECK_CTX();
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  return intra_frame(__func__, p, s, qp_source_of(p));
}

}  // extern "C"

// inter_residual.hip -- residual coding and reconstruction of every inter CU of a picture for gfx950, straight from
// the CU array (kvz_hip_inter_residual_frame): what kvz_quantize_lcu_residual (transform.c:424-482, called at
// search.c:587) does to lcu->rec, lcu->coeff and the coded-block flags, between kvz_hip_inter_recon_frame and
// kvz_hip_deblock_frame.
//
// Reference: the transform tree of kvz_quantize_lcu_residual / quantize_tr_residual (transform.c:281-482), per TU the
// rdoq-off path of kvz_quantize_residual (quant-generic.c:180-273) with cu_is_intra = 0, diagonal scan, no transform
// skip; coefficient layout xy_to_zorder (cu.h:373-410); flags as lcu_set_coeff leaves them (search.c:173-190).
//
// The TUs are never listed.  A leaf TU of width S lies at an S-aligned position and the record of its top-left SCU
// says that it is one (type, depth, tr_depth), so each transform size N gets ONE launch over a FIXED grid of "slots":
// every N-aligned position of the Y plane and of the U and V planes.  A slot reads the one record that covers it and is
// a TU of this launch or nothing; a workgroup without a TU leaves at once.  No list, no counter, no scratch memory,
// and a captured launch follows the contents of the CU array.  What this costs: a workgroup holds 256 / N neighbouring
// slots of one row and runs its barriers for all of them, so a map that mixes sizes finely idles threads
// (DESIGN.md section 5).
//
// A slot's arithmetic is quantize_residual_kernel (quant.hip) with plane addressing: N threads per TU, thread = row;
// the thread loads its row of the source and of the prediction from the planes (N bytes each), keeps both in registers
// for the reconstruction and the sums, and stores its row of coefficients (2 N bytes; the TU's rows are contiguous in
// the z-order layout, so a TU's threads store one contiguous run).
#include "inter_residual_core.h"

extern "C" {

int kvz_hip_inter_residual_frame(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                 kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                 kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                 const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         nullptr, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  return residual_frame<false>(__func__, p, nullptr, s);
}

int kvz_hip_inter_residual_frame_qp(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                    kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                    kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                    const int8_t *lcu_qp, const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  return residual_frame<false>(__func__, p, nullptr, s);
}

}  // extern "C"

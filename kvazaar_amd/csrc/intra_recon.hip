// intra_recon.hip -- prediction, residual coding and reconstruction of every intra CU of a picture for gfx950, straight
// from the CU array (kvz_hip_intra_recon_frame): what kvz_intra_recon_cu (intra.c:652-706) does to lcu->rec, lcu->coeff
// and the coded-block flags, between kvz_hip_inter_residual_frame and kvz_hip_deblock_frame.
//
// Reference: per leaf TU intra_recon_tb_leaf (intra.c:590-638) = kvz_intra_build_reference + kvz_intra_predict, then
// quantize_tr_residual (transform.c:281-406) = the rdoq-off path of kvz_quantize_residual (quant-generic.c:180-273)
// with cu_is_intra = 1 (DST for 4x4 luma) under the scan of kvz_get_scan_order (encoderstate.c:1384-1398).
//
// Dependencies.  A TU predicts from the reconstruction of the TUs before it.  It reads at most 2N pixels to its left,
// down to the end of its LCU, and at most 64 pixels above it, which at the top row of an LCU reach 32 columns into the
// above-right LCU (intra_coded_left / intra_coded_above, intra_core.h).  LCU (lx, ly) therefore needs (lx-1, ly),
// (lx-1, ly-1), (lx, ly-1) and (lx+1, ly-1) complete: the wavefront t = lx + 2 ly.  ONE LAUNCH PER WAVE, lcus_x +
// 2 (lcus_y - 1) of them whatever the map holds; the kernel boundary is the only ordering between LCUs, and no workgroup
// ever waits for another one.  Y, U and V are independent chains: a workgroup per (LCU of the wave, plane).
//
// A workgroup is ONE WAVE of 64 lanes: the work inside an LCU is a chain of up to 256 dependent TUs, and a barrier
// between the steps of a TU costs a single wave nothing.  It reads the LCU's 256 records and leaves if none is an intra
// CU (most LCUs of a P picture).  Otherwise it loads the LCU's tile of its plane into LDS, with the row above (and its
// above-right part) and the column to the left, walks the 256 SCUs in z-order and, at each leaf TU's top-left, runs
// reference -> prediction -> residual -> transform -> quantisation -> dequantisation -> inverse -> reconstruction with
// the pixels in that tile; at the end it writes the pixels of the intra CUs back.  No TU reads global memory that the
// workgroup wrote.  The walk is 256 iterations whatever the map says, everything that steers it is made wave-uniform
// (readfirstlane), and every barrier is reached by all 64 lanes: lanes beyond a TU's N rows repeat the work of row
// lane % N (identical values to identical LDS addresses) and are masked at every global access.
#include "intra_recon_core.h"

extern "C" {

int kvz_hip_intra_recon_frame(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                              kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                              kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                              kvz_hip_inter_residual_cost *costs, const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         nullptr, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  return intra_frame(__func__, p, s);
}

}  // extern "C"

// intra_recon_rdoq.hip -- kvz_hip_intra_recon_frame_rdoq: kvz_hip_intra_recon_frame_sl (intra_recon_sl.hip) with the quantiser of the
// reference at preset medium and slower: a TU wider than 4, and a 4x4 TU unless cfg.rdoq_skip, takes its levels from kvz_rdoq
// (quant-generic.c:214-221) on the context set and the state of its LCU.  The kernels are the instantiations of intra_recon_core.h that
// take rdoq_source as their last trailing argument; they have this translation unit to themselves, so that the other kernels are
// compiled as they always were, and it is compiled with -ffp-contract=off (Makefile) as rdoq.hip is.  A workgroup is one wave and one
// LCU of one plane: it stages the LCU's context set, state bytes and lambda in LDS once, and per TU runs the body of rdoq_large_kernel
// between the forward transform and the has-coefficients flag (rdoq_stage.h): level_double across the lanes, last_scanpos by a ballot,
// the recursion on lane 0, clean-up and sign hiding across the lanes.  The serial recursion lies inside every step of the wavefront.
#include "rdoq_stage.h"
#include "intra_recon_core.h"

#pragma clang fp contract(off)

extern "C" {

int kvz_hip_intra_recon_frame_rdoq(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                   kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                   kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                   kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                   const kvz_hip_scaling_tables *tables, const kvz_hip_rdoq_source *rdoq,
                                   const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!rdoq) {
    // without it, it is the entry without it, launching that entry's kernel
    return kvz_hip_intra_recon_frame_sl(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp,
                                        grid, tables, params, s);
  }
  if (const char *why = chain_rdoq_why(rdoq)) return refuse_entry(__func__, invalid_because(why).text);
  // what the _sl entry refuses: a picture that needs tables without them, and tables for a picture that says it has none
  if (!tables && params && params->scaling_list != 0) return kvzhip::invalid_arg(__func__);
  kvz_hip_chain_picture p;
  tile_source tiles;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed || (tables && !chain_tables_ok(*tables)) || !tile_source_make(p, grid, &tiles)) return kvzhip::invalid_arg(__func__);
  const rdoq_source rq = rdoq_source_of(*rdoq);
  if (tables) {
    const sl_source lists = { tables->quant, tables->dequant };
    return intra_frame(__func__, p, s, qp_source_of(p), tiles, lists, rq);
  }
  return intra_frame(__func__, p, s, qp_source_of(p), tiles, rq);
}

}  // extern "C"

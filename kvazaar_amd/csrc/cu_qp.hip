// cu_qp.hip -- the QP map of a picture whose QP changes per LCU, for gfx950 (kvz_hip_cu_qp_frame): what set_cu_qps
// (encoderstate.c:550-609) leaves in cu_array->qp for the deblocking filter (get_qp_y_pred, filter.c:263-282), and the QP
// predictor of every LCU that the entropy coder codes cu_qp_delta against (encode_coding_tree.c:511-529), between
// kvz_hip_intra_recon_frame_qp and kvz_hip_deblock_frame with per_cu_qp = 1.
//
// Reference: set_cu_qps with max_qp_delta_depth == 0 -- the quantization group is the LCU -- over kvz_get_cu_ref_qp
// (encoderstate.c:1408-1430) and is_last_cu_in_qg (encoderstate.h:332-342).  With the group at the LCU's corner both predictors of
// kvz_get_cu_ref_qp are last_qp, so a CU before the first coded CU of its LCU gets last_qp, the first coded CU and every CU after
// it keep the LCU's QP (prev_qp >= 0 from there on), and *last_qp = cu->qp at the group's last CU stores the LCU's QP if the LCU
// has a coded CU and last_qp itself otherwise.  A ragged edge can make is_last_cu_in_qg true for more than one CU; each such store
// writes one of these two values in the same order, so the rule holds there too (the header states the derivation in full).
//
// Three launches of fixed shape, no atomics:
//   1. per LCU: the z-order index of its first coded CU; lcu_last_qp[lcu] = the LCU's QP if there is one, else -1
//   2. per chain: the exclusive scan "QP of the last LCU before this one that has a coded CU, else start_qp" over lcu_last_qp,
//      in place -- one workgroup per chain walks it in runs of 256 with a carry
//   3. per LCU: the first coded CU again (256 records and flags, cheaper than a buffer the call would have to own) and the qp byte
//      of every SCU
#include "cu_qp_core.h"

extern "C" {

int kvz_hip_cu_qp_frame(kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp, int8_t *lcu_last_qp,
                        const kvz_hip_cu_qp_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!params) return kvzhip::invalid_arg(__func__);
  // the chains of this entry alone, which the record cannot say: raster runs of chain_lcus LCUs, whole LCU rows
  const kvz_hip_cu_qp_tiles_params rows = { params->start_qp, 0 };
  kvz_hip_filter_picture p;
  if (!cu_qp_pack(&p, cus, cbf, width, height, lcu_qp, lcu_last_qp, nullptr, &rows) || !cu_qp_arrays_ok(p) || !picture_ok(width, height) || !cu_qp_chains_ok(p))
    return kvzhip::invalid_arg(__func__);
  const int lcus_x = (width + 63) >> 6, n_lcu = lcus_x * ((height + 63) >> 6);
  if (params->chain_lcus < 0 || params->chain_lcus % lcus_x) return kvzhip::invalid_arg(__func__);
  const int chain = params->chain_lcus ? params->chain_lcus : n_lcu;
  // the launch sequence depends on width, height and chain_lcus alone
  return cu_qp_launch(p, s, dim3((unsigned)((n_lcu + chain - 1) / chain)), n_lcu, chain);
}

}  // extern "C"

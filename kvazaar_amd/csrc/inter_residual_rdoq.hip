// inter_residual_rdoq.hip -- kvz_hip_inter_residual_frame_rdoq: kvz_hip_inter_residual_frame_sl (inter_residual_sl.hip) with the quantiser
// of the reference at preset medium and slower: a TU wider than 4, and a 4x4 TU unless cfg.rdoq_skip, takes its levels from kvz_rdoq
// (quant-generic.c:214-221) on the context set and the state of its LCU.  The arrays of kvz_rdoq's recursion take about 50 KB of LDS
// per TU (rdoq_stage.h), so the 256 / N TUs of a workgroup of inter_residual_tu_kernel do not fit: the kernel here gives a TU a wave
// of its own, in the manner of the quantise half of intra_tu (intra_recon_core.h).  The slots, the CU rule, the constants of a TU,
// the coefficient layout, the flags and the sums are those of inter_residual_tu_kernel; a slot that is no TU leaves at once.  Between
// the forward transform and the has-coefficients flag the wave runs the body of rdoq_large_kernel: level_double across the lanes,
// last_scanpos by a ballot, the recursion on lane 0, clean-up and sign hiding across the lanes.  With rdoq_skip the 4x4 launch is the
// instantiation of inter_residual_tu_kernel that the entry without RDOQ launches.  This translation unit is compiled with
// -ffp-contract=off (Makefile), as rdoq.hip is.  The kernel itself stands in inter_residual_rdoq_core.h, which the multi-picture
// entry (inter_residual_multi_rdoq.hip) shares; here it is instantiated for one picture, to the instructions it had.
#include "inter_residual_rdoq_core.h"

#pragma clang fp contract(off)

namespace {

template <int N, bool SL>
void launch_rdoq_size(const resid_args &a, int chroma, hipStream_t st, const lcu_qp_source &q, const sl_source &t, const rdoq_source &r)
{
  const resid_slots n = residual_slots<N>(a.width, a.height, chroma);
  hipLaunchKernelGGL((inter_residual_rdoq_kernel<N, SL, resid_args>), dim3((unsigned)(n.n_y + 2 * n.n_c)), dim3(64), 0, st, a, n.nx_y, n.n_y, n.nx_c, n.n_c, q, t, r);
}

// the record checked as residual_frame checks it; one launch per size, 32 down to 4, behind the init kernel
template <bool SL>
int residual_rdoq_frame(const char *entry, const kvz_hip_chain_picture &p, const kvz_hip_scaling_tables *tables, const rdoq_source &r, kvz_hip_stream s)
{
  if (!chain_picture_args_ok(p, false, SL) || (SL && !chain_tables_ok(*tables)) || !chain_one_qp_ok(p)) return kvzhip::invalid_arg(entry);
  const int chroma = p.params.chroma ? 1 : 0;
  const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
  quant_consts ky = {}, kc = {};                                              // read by the 4x4 kernel without a trailing source only
  if (!SL && !p.lcu_qp) {
    // one QP and flat lists: what the one-QP entry refuses (make_consts per size, quant_core.h)
    for (int n = 32; n >= 4; n >>= 1)
      if (!make_consts(&qp, n, 0, 0, &ky) || !make_consts(&qp, n, 2, 2, &kc)) return kvzhip::invalid_arg(entry);
  }
  resid_args a;
  fill(a, p);
  hipStream_t st = ctx_stream(s);
  if (int e = residual_init(a, st)) return e;
  const lcu_qp_source per_lcu = qp_source_of(p);
  const sl_source lists = { SL ? tables->quant : nullptr, SL ? tables->dequant : nullptr, p.params.qp };
  launch_rdoq_size<32, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_size<16, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_size<8, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  if (!r.skip) {
    launch_rdoq_size<4, SL>(a, chroma, st, per_lcu, lists, r);
    KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  } else {
    // every 4x4 TU keeps the plain quantiser: the 4x4 launch of the entry without RDOQ
    if constexpr (SL) launch_size<4>(a, ky, kc, chroma, st, per_lcu, lists);
    else if (p.lcu_qp) launch_size<4>(a, ky, kc, chroma, st, per_lcu);
    else launch_size<4>(a, ky, kc, chroma, st);                              // ky, kc: make_consts of size 4, the last made above
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frame_rdoq(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                      kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                      kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                      const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables, const kvz_hip_rdoq_source *rdoq,
                                      const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!rdoq) {
    // without it, it is the entry without it, launching that entry's kernels
    return kvz_hip_inter_residual_frame_sl(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, tables,
                                           params, s);
  }
  if (const char *why = chain_rdoq_why(rdoq)) return refuse_entry(__func__, invalid_because(why).text);
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  // without tables, what the _sl entry refuses without them is refused: scaling_list says whether tables are given
  if (tables) return residual_rdoq_frame<true>(__func__, p, tables, rdoq_source_of(*rdoq), s);
  return residual_rdoq_frame<false>(__func__, p, nullptr, rdoq_source_of(*rdoq), s);
}

}  // extern "C"

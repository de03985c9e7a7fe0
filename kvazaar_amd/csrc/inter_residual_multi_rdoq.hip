// inter_residual_multi_rdoq.hip -- kvz_hip_inter_residual_frames_rdoq: kvz_hip_inter_residual_frame_rdoq (inter_residual_rdoq.hip) for
// up to sixteen pictures that do not depend on each other, in one call: the single entry's launches -- one per TU width, and the init
// launch where a picture has cbf_out or costs -- each covering all pictures, the picture being the grid's second dimension.
//
// The kernel is inter_residual_rdoq_kernel (inter_residual_rdoq_core.h) with the table of per-picture records as its argument
// (resid_batch_rdoq), behind init_pictures_kernel (frame_sources.h) on the same table: a wave per TU, the slot at blockIdx.x and the
// picture at blockIdx.y.  The wave reads its picture's record from the kernel arguments with scalar loads, counts that picture's
// slots itself (a slot beyond them leaves at once) and builds the sources of the single-picture kernel from the record -- every
// picture has its own context sets, states and set index per LCU; the RDOQ tables and rdoq_skip are the call's.  From there on it is
// the single-picture kernel's code, hence the same bytes.  With rdoq_skip every 4x4 TU keeps the plain quantiser: that launch is the
// 4x4 launch of kvz_hip_inter_residual_frames_ts on the same records.  The records are checked by the walk that the six
// multi-picture entries of the residual stages share (chain_records_why, chain_host.h).  This translation unit is compiled with
// -ffp-contract=off (Makefile), as rdoq.hip is.
#include "inter_residual_rdoq_core.h"

#pragma clang fp contract(off)

namespace {

template <int N, bool SL>
void launch_rdoq_pictures(const resid_batch_rdoq &b, int n_pictures, hipStream_t st)
{
  int slots = 0;
  for (int i = 0; i < n_pictures; ++i) {
    const resid_slots n = residual_slots<N>(b.p[i].width, b.p[i].height, b.p[i].chroma);
    slots = max(slots, n.n_y + 2 * n.n_c);
  }
  const lcu_qp_source no_qp = {};                                             // not read: every wave makes its own of its picture's record
  const sl_source no_lists = {};
  const rdoq_source no_rdoq = {};
  hipLaunchKernelGGL((inter_residual_rdoq_kernel<N, SL, resid_batch_rdoq>), dim3((unsigned)slots, (unsigned)n_pictures), dim3(64), 0, st, b, 0, 0, 0, 0, no_qp,
                     no_lists, no_rdoq);
}

// one launch per size, 32 down to 4; plain: the records as kvz_hip_inter_residual_frames_ts takes them, read with rdoq_skip only
template <bool SL>
int launch_all(const resid_batch_rdoq &b, const resid_batch_ts_data &plain, int n_pictures, hipStream_t st)
{
  launch_rdoq_pictures<32, SL>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_pictures<16, SL>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_pictures<8, SL>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  if (!b.skip) {
    launch_rdoq_pictures<4, SL>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  } else {
    // every 4x4 TU keeps the plain quantiser: the 4x4 launch of the multi-picture entry without RDOQ
    resid_batch_ts<SL, false> typed;
    static_cast<resid_batch_ts_data &>(typed) = plain;
    launch_pictures<4>(typed, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frames_rdoq(const kvz_hip_chain_picture_rdoq *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  bool any = false;
  for (int i = 0; i < n_pictures; ++i) any = any || pictures[i].rdoq;
  if (!any) {
    // no record carries rdoq: the entry without it on the same fields (the stage does not depend on tiles), launching that entry's kernels
    kvz_hip_chain_picture_ts plain[KVZ_HIP_MAX_CHAIN_PICTURES];
    for (int i = 0; i < n_pictures; ++i) plain[i] = { pictures[i].pic, nullptr, pictures[i].tables, nullptr, nullptr };
    return kvz_hip_inter_residual_frames_ts(plain, n_pictures, s);
  }
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, false, nullptr, &plan, &at)) return refuse_picture(__func__, at, why);
  const kvz_hip_rdoq_source *first = pictures[0].rdoq;                          // not NULL: some record carries one and the call is homogeneous
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant;
  resid_batch_rdoq b;
  resid_batch_ts_data plain;
  __builtin_memset(&b, 0, sizeof b);
  __builtin_memset(&plain, 0, sizeof plain);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_rdoq &r = pictures[i];
    fill(b.p[i], r.pic, r.pic.params.qp);                                       // the slot clamps it with tables only, as the single entry
    fill_lists(b.p[i], r.tables);
    fill_rdoq(b.p[i], *r.rdoq);
    fill(plain.p[i], r.pic, lists ? clip_lcu_qp(r.pic.params.qp) : r.pic.params.qp);   // as kvz_hip_inter_residual_frames_ts fills it
    fill_lists(plain.p[i], r.tables);
  }
  b.quant = first->tables.quant; b.err_scale = first->tables.err_scale; b.skip = first->rdoq_skip != 0;
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags, rdoq_skip and the presence of cbf_out / costs alone
  if (int e = init_pictures<inter_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  return lists ? launch_all<true>(b, plain, n_pictures, st) : launch_all<false>(b, plain, n_pictures, st);
}

}  // extern "C"

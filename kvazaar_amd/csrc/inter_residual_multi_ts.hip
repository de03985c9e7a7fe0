// inter_residual_multi_ts.hip -- kvz_hip_inter_residual_frames_ts: kvz_hip_inter_residual_frame_ts (inter_residual_ts.hip) for up to
// sixteen pictures that do not depend on each other, in one call: the single entry's launches -- one per transform size, and the init
// launch where a picture has cbf_out or costs -- each covering all pictures, the picture being the grid's second dimension.
//
// The kernels are the instantiations of inter_residual_core.h, and of init_pictures_kernel (frame_sources.h), whose argument is the
// table of per-picture records with the tables and the transform-skip source of each picture (resid_batch_ts<SL, TS>).  SL and TS
// select the code of a TU, so a call is homogeneous in them and the table's type says which kernel runs; as in the single entry only
// the 4x4 launch runs the two trials, the launches of the other sizes are those of the call without transform skip.  They have this
// translation unit to themselves, so that the other kernels are compiled as they always were.  A workgroup reads its picture's record
// from the kernel arguments with scalar loads; a TU derives its constants with flat_consts / sl_consts from the record's lcu_qp or qp
// as the single-picture kernels do, hence the same bytes.  The records are checked by the walk that the six multi-picture entries of
// the residual stages share (chain_records_why, chain_host.h).
#include "inter_residual_core.h"

static_assert(sizeof(kvz_hip_chain_picture_ts) == 200 && sizeof(kvz_hip_trskip) == 16, "layouts documented in kvz_hip.h");

namespace {

// the records under the type that says which kernel runs
template <bool SL, bool TS>
resid_batch_ts<SL, TS> typed(const resid_batch_ts_data &d)
{
  resid_batch_ts<SL, TS> b;
  static_cast<resid_batch_ts_data &>(b) = d;
  return b;
}

// one launch per size, 32 down to 4; the three larger sizes are the kernels of the call without transform skip, on these records
template <bool SL>
int launch_all(const resid_batch_ts_data &b, bool skip, int n_pictures, hipStream_t st)
{
  launch_pictures<32>(typed<SL, false>(b), n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  launch_pictures<16>(typed<SL, false>(b), n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  launch_pictures<8>(typed<SL, false>(b), n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  if constexpr (SL) {
    if (skip) launch_pictures<4>(typed<true, true>(b), n_pictures, st);
    else launch_pictures<4>(typed<true, false>(b), n_pictures, st);
  } else {
    // a call with flat lists is here for transform skip: with neither option it went to the plainer entry
    launch_pictures<4>(typed<false, true>(b), n_pictures, st);
  }
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frames_ts(const kvz_hip_chain_picture_ts *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  bool options = false;
  for (int i = 0; i < n_pictures; ++i) options = options || pictures[i].tables.quant || pictures[i].tables.dequant || pictures[i].ts;
  if (!options) {
    // neither tables nor transform skip (the stage does not depend on tiles): the entry without them on the embedded records
    kvz_hip_chain_picture plain[KVZ_HIP_MAX_CHAIN_PICTURES];
    for (int i = 0; i < n_pictures; ++i) plain[i] = pictures[i].pic;
    return kvz_hip_inter_residual_frames(plain, n_pictures, s);
  }
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, false, nullptr, &plan, &at)) return refuse_picture(__func__, at, why);
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant, skip = pictures[0].ts != nullptr;
  resid_batch_ts_data b;
  __builtin_memset(&b, 0, sizeof b);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_ts &r = pictures[i];
    fill(b.p[i], r.pic, lists ? clip_lcu_qp(r.pic.params.qp) : r.pic.params.qp);   // as the single-picture kernels: clamped with tables only
    fill_lists(b.p[i], r.tables);
    fill_trskip(b.p[i], r.ts, r.tr_skip_out);
  }
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (int e = init_pictures<inter_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  return lists ? launch_all<true>(b, skip, n_pictures, st) : launch_all<false>(b, skip, n_pictures, st);
}

}  // extern "C"

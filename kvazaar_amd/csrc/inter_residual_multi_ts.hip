// inter_residual_multi_ts.hip -- kvz_hip_inter_residual_frames_ts: kvz_hip_inter_residual_frame_ts (inter_residual_ts.hip) for up to
// sixteen pictures that do not depend on each other, in one call: the single entry's launches -- one per transform size, and the init
// launch where a picture has cbf_out or costs -- each covering all pictures, the picture being the grid's second dimension.
//
// The kernels are the instantiations of inter_residual_core.h whose argument is the table of per-picture records with the tables and
// the transform-skip source of each picture (resid_batch_ts<SL, TS>).  SL and TS select the code of a TU, so a call is homogeneous in
// them and the table's type says which kernel runs; as in the single entry only the 4x4 launch runs the two trials, the launches of
// the other sizes are those of the call without transform skip.  They have this translation unit to themselves, so that the other
// kernels are compiled as they always were.  A workgroup reads its picture's record from the kernel arguments with scalar loads; a TU
// derives its constants with flat_consts / sl_consts from the record's lcu_qp or qp as the single-picture kernels do, hence the same
// bytes.
#include "inter_residual_core.h"

static_assert(sizeof(kvz_hip_chain_picture_ts) == 200 && sizeof(kvz_hip_trskip) == 16, "layouts documented in kvz_hip.h");

namespace {

// inter_residual_init_kernel for every picture that has cbf_out or costs: grid (blocks of the largest such picture, pictures)
__global__ __launch_bounds__(256) void inter_residual_init_multi_ts_kernel(resid_batch_ts_data b)
{
  const resid_pic_ts &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  zero_cu_outputs(a, i, inter_cu_rule());
}

// the records under the type that says which kernel runs
template <bool SL, bool TS>
resid_batch_ts<SL, TS> typed(const resid_batch_ts_data &d)
{
  resid_batch_ts<SL, TS> b;
  static_cast<resid_batch_ts_data &>(b) = d;
  return b;
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
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant, skip = pictures[0].ts != nullptr;
  resid_batch_ts_data b;
  __builtin_memset(&b, 0, sizeof b);
  int init_scus = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_ts &r = pictures[i];
    const kvz_hip_chain_picture &p = r.pic;
    const char *why = chain_record_ts_why(pictures, i, false, lists, skip);
    if (!why) why = chain_record_ts_shared(pictures, i);
    if (why) return refuse_picture(__func__, i, why);
    resid_pic_ts &a = b.p[i];
    fill(a, p, lists ? clip_lcu_qp(p.params.qp) : p.params.qp);                 // as the single-picture kernels: clamped with tables only
    if (lists) { a.quant = r.tables.quant; a.dequant = r.tables.dequant; }
    if (r.ts) { a.lcu_bit_cost = r.ts->lcu_bit_cost; a.tr_skip_out = r.tr_skip_out; a.bit_cost = r.ts->bit_cost; }
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (p.src.width >> 2) * (p.src.height >> 2));
  }
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(inter_residual_init_multi_ts_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("inter_residual_init_multi_ts_kernel");
  }
  if (lists) {
    launch_pictures<32>(typed<true, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<16>(typed<true, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<8>(typed<true, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    if (skip) launch_pictures<4>(typed<true, true>(b), n_pictures, st);
    else launch_pictures<4>(typed<true, false>(b), n_pictures, st);
  } else {
    // transform skip with flat lists: the three larger sizes are the kernels of the call without it, on these records
    launch_pictures<32>(typed<false, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<16>(typed<false, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<8>(typed<false, false>(b), n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<4>(typed<false, true>(b), n_pictures, st);
  }
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

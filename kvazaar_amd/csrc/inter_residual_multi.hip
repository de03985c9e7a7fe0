// inter_residual_multi.hip -- kvz_hip_inter_residual_frames: kvz_hip_inter_residual_frame_qp (inter_residual.hip) for up to sixteen
// pictures that do not depend on each other, in one call: the single entry's launches -- one per transform size, and the init launch
// where a picture has cbf_out or costs -- each covering all pictures, the picture being the grid's second dimension.  The stage is
// bound by its launches, so what a host with P pictures gains is the launches it no longer repeats.
//
// The kernels are the instantiations of inter_residual_core.h, and of init_pictures_kernel (frame_sources.h), whose argument is the
// table of per-picture records (resid_batch); they have this translation unit to themselves, so that the single-picture kernels are
// compiled as they always were.  A workgroup reads its picture's record from the kernel arguments with scalar loads; a TU derives its
// constants with flat_consts from the record's lcu_qp or qp: the function the host uses for the one-QP kernels and the per-LCU kernels
// use on the device, hence the same bytes.  The records are checked by the walk that the six multi-picture entries of the residual
// stages share (chain_records_why, chain_host.h).
#include "inter_residual_core.h"

extern "C" {

int kvz_hip_inter_residual_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, false, nullptr, &plan, &at)) return refuse_picture(__func__, at, why);
  resid_batch b;
  __builtin_memset(&b, 0, sizeof b);
  for (int i = 0; i < n_pictures; ++i) fill(b.p[i], pictures[i], pictures[i].params.qp);
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (int e = init_pictures<inter_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  launch_pictures<32>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  launch_pictures<16>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  launch_pictures<8>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  launch_pictures<4>(b, n_pictures, st);
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

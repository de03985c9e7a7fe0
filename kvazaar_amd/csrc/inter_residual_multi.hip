// inter_residual_multi.hip -- kvz_hip_inter_residual_frames: kvz_hip_inter_residual_frame_qp (inter_residual.hip) for up to sixteen
// pictures that do not depend on each other, in one call: the single entry's launches -- one per transform size, and the init launch
// where a picture has cbf_out or costs -- each covering all pictures, the picture being the grid's second dimension.  The stage is
// bound by its launches, so what a host with P pictures gains is the launches it no longer repeats.
//
// The kernels are the instantiations of inter_residual_core.h whose argument is the table of per-picture records (resid_batch); they
// have this translation unit to themselves, so that the single-picture kernels are compiled as they always were.  A workgroup reads
// its picture's record from the kernel arguments with scalar loads; a TU derives its constants with flat_consts from the record's
// lcu_qp or qp: the function the host uses for the one-QP kernels and the per-LCU kernels use on the device, hence the same bytes.
#include "inter_residual_core.h"

namespace {

// inter_residual_init_kernel for every picture that has cbf_out or costs: grid (blocks of the largest such picture, pictures)
__global__ __launch_bounds__(256) void inter_residual_init_multi_kernel(resid_batch b)
{
  const resid_pic &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  zero_cu_outputs(a, i, inter_cu_rule());
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  resid_batch b;
  __builtin_memset(&b, 0, sizeof b);
  int init_scus = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture &p = pictures[i];
    if (const char *why = chain_record_why(pictures, i, false)) return refuse_picture(__func__, i, why);
    fill(b.p[i], p, p.params.qp);
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (p.src.width >> 2) * (p.src.height >> 2));
  }
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(inter_residual_init_multi_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("inter_residual_init_multi_kernel");
  }
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

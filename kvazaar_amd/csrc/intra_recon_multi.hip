// intra_recon_multi.hip -- kvz_hip_intra_recon_frames: kvz_hip_intra_recon_frame_qp (intra_recon_qp.hip) for up to sixteen pictures
// that do not depend on each other, in one call.  A launch of the single-picture entry is one wave per LCU row and plane -- at most
// 51 waves at 1080p on a device with a thousand SIMDs -- and the launches of a picture depend on each other, so the device is
// filled from the side: launch t holds wave t of every picture, the picture being the grid's third dimension, and the call makes
// as many dependent launches as its largest picture alone.  What tiles do inside a picture (intra_recon_tiles.hip), between pictures.
//
// The kernel is the instantiation of intra_recon_core.h whose argument is the table of per-picture records (intra_batch); it has this
// translation unit to itself, so that the single-picture kernels are compiled as they always were.  A workgroup reads its picture's
// record from the kernel arguments with scalar loads and derives its LCU's constants with flat_consts from the record's lcu_qp or qp:
// the function the host uses for the one-QP kernel and the per-LCU kernel uses on the device, hence the same bytes as either.
#include "intra_recon_core.h"

namespace {

// intra_recon_init_kernel for every picture that has cbf_out or costs: grid (blocks of the largest such picture, pictures)
__global__ __launch_bounds__(256) void intra_recon_init_multi_kernel(intra_batch b)
{
  const intra_pic &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  zero_cu_outputs(a, i, intra_cu_rule());
}

}  // namespace

extern "C" {

int kvz_hip_intra_recon_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  intra_batch b;
  __builtin_memset(&b, 0, sizeof b);
  int waves = 0, groups = 0, planes = 1, init_scus = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture &p = pictures[i];
    if (const char *why = chain_record_why(pictures, i, true)) return refuse_picture(__func__, i, why);
    intra_pic &a = b.p[i];
    fill(a, p, p.params.qp);
    const int lcus_y = (a.height + 63) >> 6;
    waves = max(waves, a.lcus_x + 2 * (lcus_y - 1));
    groups = max(groups, lcus_y);
    if (a.chroma) planes = 3;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (a.width >> 2) * (a.height >> 2));
  }
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(intra_recon_init_multi_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("intra_recon_init_multi_kernel");
  }
  for (int t = 0; t < waves; ++t) {
    hipLaunchKernelGGL((intra_recon_wave_kernel<intra_batch>), dim3((unsigned)groups, (unsigned)planes, (unsigned)n_pictures), dim3(WG), 0, st, b, t);
    KVZ_CHECK_LAUNCH("intra_recon_wave_kernel");
  }
  return KVZ_HIP_OK;
}

}  // extern "C"

// intra_recon_multi.hip -- kvz_hip_intra_recon_frames: kvz_hip_intra_recon_frame_qp (intra_recon_qp.hip) for up to sixteen pictures
// that do not depend on each other, in one call.  A launch of the single-picture entry is one wave per LCU row and plane -- at most
// 51 waves at 1080p on a device with a thousand SIMDs -- and the launches of a picture depend on each other, so the device is
// filled from the side: launch t holds wave t of every picture, the picture being the grid's third dimension, and the call makes
// as many dependent launches as its largest picture alone.  What tiles do inside a picture (intra_recon_tiles.hip), between pictures.
//
// The kernel is the instantiation of intra_recon_core.h whose argument is the table of per-picture records (intra_batch), behind
// init_pictures_kernel (frame_sources.h) on the same table; they have this translation unit to themselves, so that the single-picture
// kernels are compiled as they always were.  A workgroup reads its picture's record from the kernel arguments with scalar loads and
// derives its LCU's constants with flat_consts from the record's lcu_qp or qp: the function the host uses for the one-QP kernel and
// the per-LCU kernel uses on the device, hence the same bytes as either.  The records are checked, and the launches sized, by the
// walk that the six multi-picture entries of the residual stages share (chain_records_why, chain_host.h): a picture of this entry is
// one tile.
#include "intra_recon_core.h"

extern "C" {

int kvz_hip_intra_recon_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  chain_tiles tiles;
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, true, &tiles, &plan, &at)) return refuse_picture(__func__, at, why);
  intra_batch b;
  __builtin_memset(&b, 0, sizeof b);
  for (int i = 0; i < n_pictures; ++i) fill(b.p[i], pictures[i], pictures[i].params.qp);
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (int e = init_pictures<intra_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  for (int t = 0; t < plan.waves; ++t) {
    hipLaunchKernelGGL((intra_recon_wave_kernel<intra_batch>), dim3((unsigned)plan.groups, (unsigned)plan.planes, (unsigned)n_pictures), dim3(WG), 0, st, b, t);
    KVZ_CHECK_LAUNCH("intra_recon_wave_kernel");
  }
  return KVZ_HIP_OK;
}

}  // extern "C"

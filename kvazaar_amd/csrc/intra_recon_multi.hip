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
  const int sy = i / a.cus_stride, sx = i - sy * a.cus_stride;
  int cu_x, cu_y, leaf;
  if (!intra_cu_of(a.cus[(size_t)i * 5], 4 * sx, 4 * sy, a.width, a.height, cu_x, cu_y, leaf)) return;
  if (a.cbf_out) a.cbf_out[i] = 0;
  if (a.cost && cu_x == 4 * sx && cu_y == 4 * sy) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a.cost[(size_t)i * 6 + j] = 0u;
  }
}

int refuse(const char *entry, int i)
{
  char msg[160];
  snprintf(msg, sizeof msg, "%s: invalid argument in picture %d (null or misaligned buffer, size or parameter out of range, or an output shared with "
           "another picture)", entry, i);
  kvzhip::set_error_msg(msg);
  return KVZ_HIP_ERR_INVALID;
}

}  // namespace

extern "C" {

int kvz_hip_intra_recon_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (n_pictures == 0) return KVZ_HIP_OK;
  if (!pictures || n_pictures < 0 || n_pictures > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__);
  intra_batch b;
  __builtin_memset(&b, 0, sizeof b);
  int waves = 0, groups = 0, planes = 1, init_scus = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture &p = pictures[i];
    if (!intra_frame_args_ok(&p.src, p.rec_y, p.stride_y, p.rec_u, p.rec_v, p.stride_c, p.cus, p.intra_modes, p.coeff_y, p.coeff_u, p.coeff_v, p.costs,
                             &p.params, false))
      return refuse(__func__, i);
    // one QP for the picture: what the one-QP entry refuses
    const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
    quant_consts k;
    if (!p.lcu_qp && (!make_consts(&qp, 4, 0, 0, &k) || !make_consts(&qp, 4, 2, 2, &k))) return refuse(__func__, i);
    for (int j = 0; j < i; ++j)
      if (p.rec_y == pictures[j].rec_y || p.cus == pictures[j].cus || p.coeff_y == pictures[j].coeff_y) return refuse(__func__, i);
    const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
    intra_pic &a = b.p[i];
    a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
    a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
    a.src_stride[0] = p.src.stride_y; a.src_stride[1] = a.src_stride[2] = p.src.stride_c;
    a.rec_stride[0] = p.stride_y; a.rec_stride[1] = a.rec_stride[2] = p.stride_c;
    a.coeff[0] = p.coeff_y; a.coeff[1] = chroma ? p.coeff_u : nullptr; a.coeff[2] = chroma ? p.coeff_v : nullptr;
    a.cus = (u32 *)p.cus; a.modes = p.intra_modes; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
    a.qp = p.params.qp;
    a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
    a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
    const int lcus_y = (height + 63) >> 6;
    waves = max(waves, a.lcus_x + 2 * (lcus_y - 1));
    groups = max(groups, lcus_y);
    if (chroma) planes = 3;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (width >> 2) * (height >> 2));
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

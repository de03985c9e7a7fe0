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
  const int sy = i / a.cus_stride, sx = i - sy * a.cus_stride;
  int cu_x, cu_y, leaf;
  if (!inter_cu_at(a, 4 * sx, 4 * sy, cu_x, cu_y, leaf)) return;
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

// workgroups of the launch of size N for the picture with the most slots (launch_size, inter_residual_core.h)
template <int N>
void launch_pictures(const resid_batch &b, int n_pictures, hipStream_t st)
{
  constexpr int TPB = 256 / N;
  int groups = 0;
  for (int i = 0; i < n_pictures; ++i) {
    const resid_pic &a = b.p[i];
    const int nx_y = (a.width + N - 1) / N, n_y = nx_y * ((a.height + N - 1) / N);
    const int nx_c = ((a.width >> 1) + N - 1) / N, n_c = (a.chroma && N < 32) ? nx_c * (((a.height >> 1) + N - 1) / N) : 0;
    groups = max(groups, (n_y + 2 * n_c + TPB - 1) / TPB);
  }
  const quant_consts none = {};                                               // not read: every TU derives its own
  hipLaunchKernelGGL((inter_residual_tu_kernel<N, resid_batch>), dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, st, b, none, none, 0, 0, 0, 0);
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (n_pictures == 0) return KVZ_HIP_OK;
  if (!pictures || n_pictures < 0 || n_pictures > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__);
  resid_batch b;
  __builtin_memset(&b, 0, sizeof b);
  int init_scus = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture &p = pictures[i];
    if (!residual_frame_args_ok(&p.src, p.rec_y, p.stride_y, p.rec_u, p.rec_v, p.stride_c, p.cus, p.coeff_y, p.coeff_u, p.coeff_v, p.costs, &p.params, false))
      return refuse(__func__, i);
    // one QP for the picture: what the one-QP entry refuses
    const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
    quant_consts k;
    if (!p.lcu_qp && (!make_consts(&qp, 4, 0, 0, &k) || !make_consts(&qp, 4, 2, 2, &k))) return refuse(__func__, i);
    for (int j = 0; j < i; ++j)
      if (p.rec_y == pictures[j].rec_y || p.cus == pictures[j].cus || p.coeff_y == pictures[j].coeff_y) return refuse(__func__, i);
    const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
    resid_pic &a = b.p[i];
    a.src_y = p.src.y; a.src_u = chroma ? p.src.u : nullptr; a.src_v = chroma ? p.src.v : nullptr;
    a.rec_y = p.rec_y; a.rec_u = chroma ? p.rec_u : nullptr; a.rec_v = chroma ? p.rec_v : nullptr;
    a.src_stride_y = p.src.stride_y; a.src_stride_c = p.src.stride_c; a.rec_stride_y = p.stride_y; a.rec_stride_c = p.stride_c;
    a.coeff_y = p.coeff_y; a.coeff_u = chroma ? p.coeff_u : nullptr; a.coeff_v = chroma ? p.coeff_v : nullptr;
    a.cus = (u32 *)p.cus; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
    a.qp = p.params.qp;
    a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
    a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (width >> 2) * (height >> 2));
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

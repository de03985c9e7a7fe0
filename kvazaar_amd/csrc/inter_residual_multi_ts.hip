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
  const int sy = i / a.cus_stride, sx = i - sy * a.cus_stride;
  int cu_x, cu_y, leaf;
  if (!inter_cu_at(a, 4 * sx, 4 * sy, cu_x, cu_y, leaf)) return;
  if (a.cbf_out) a.cbf_out[i] = 0;
  if (a.cost && cu_x == 4 * sx && cu_y == 4 * sy) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a.cost[(size_t)i * 6 + j] = 0u;
  }
}

int refuse(const char *entry, int i, const char *why)
{
  char msg[200];
  snprintf(msg, sizeof msg, "%s: invalid argument in picture %d (%s)", entry, i, why);
  kvzhip::set_error_msg(msg);
  return KVZ_HIP_ERR_INVALID;
}

// workgroups of the launch of size N for the picture with the most slots (launch_size, inter_residual_core.h)
template <int N, bool SL, bool TS>
void launch_pictures(const resid_batch_ts_data &d, int n_pictures, hipStream_t st)
{
  constexpr int TPB = 256 / N;
  int groups = 0;
  for (int i = 0; i < n_pictures; ++i) {
    const resid_pic_ts &a = d.p[i];
    const int nx_y = (a.width + N - 1) / N, n_y = nx_y * ((a.height + N - 1) / N);
    const int nx_c = ((a.width >> 1) + N - 1) / N, n_c = (a.chroma && N < 32) ? nx_c * (((a.height >> 1) + N - 1) / N) : 0;
    groups = max(groups, (n_y + 2 * n_c + TPB - 1) / TPB);
  }
  resid_batch_ts<SL, TS> b;
  static_cast<resid_batch_ts_data &>(b) = d;
  const quant_consts none = {};                                               // not read: every TU derives its own
  hipLaunchKernelGGL((inter_residual_tu_kernel<N, resid_batch_ts<SL, TS>>), dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, st, b, none, none, 0, 0, 0,
                     0);
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frames_ts(const kvz_hip_chain_picture_ts *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (n_pictures == 0) return KVZ_HIP_OK;
  if (!pictures || n_pictures < 0 || n_pictures > KVZ_HIP_MAX_CHAIN_PICTURES) return kvzhip::invalid_arg(__func__);
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
    const bool has_lists = r.tables.quant || r.tables.dequant;
    if (has_lists != lists || (r.ts != nullptr) != skip)
      return refuse(__func__, i, "a call is homogeneous: every record carries tables or none does, every record carries ts or none does");
    if (has_lists && (!r.tables.quant || !r.tables.dequant || (((uintptr_t)r.tables.quant | (uintptr_t)r.tables.dequant) & 15)))
      return refuse(__func__, i, "a table is null or not 16-byte aligned");
    if (!residual_frame_args_ok(&p.src, p.rec_y, p.stride_y, p.rec_u, p.rec_v, p.stride_c, p.cus, p.coeff_y, p.coeff_u, p.coeff_v, p.costs, &p.params, has_lists))
      return refuse(__func__, i, "null or misaligned buffer, size or parameter out of range, or scaling_list does not say whether tables are given");
    if (r.ts && (!r.tr_skip_out || (!r.ts->lcu_bit_cost && r.ts->bit_cost < 0) || ((uintptr_t)r.ts->lcu_bit_cost & 3)))
      return refuse(__func__, i, "ts without tr_skip_out, a negative bit_cost without lcu_bit_cost, or a misaligned lcu_bit_cost");
    // one QP for the picture: what the one-QP entry refuses
    if (!p.lcu_qp && p.params.qp < 0) return refuse(__func__, i, "a negative qp without lcu_qp");
    for (int j = 0; j < i; ++j) {
      const kvz_hip_chain_picture &o = pictures[j].pic;
      if (p.rec_y == o.rec_y || p.cus == o.cus || p.coeff_y == o.coeff_y || (r.ts && r.tr_skip_out == pictures[j].tr_skip_out))
        return refuse(__func__, i, "an output shared with another picture");
    }
    const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
    resid_pic_ts &a = b.p[i];
    a.src_y = p.src.y; a.src_u = chroma ? p.src.u : nullptr; a.src_v = chroma ? p.src.v : nullptr;
    a.rec_y = p.rec_y; a.rec_u = chroma ? p.rec_u : nullptr; a.rec_v = chroma ? p.rec_v : nullptr;
    a.src_stride_y = p.src.stride_y; a.src_stride_c = p.src.stride_c; a.rec_stride_y = p.stride_y; a.rec_stride_c = p.stride_c;
    a.coeff_y = p.coeff_y; a.coeff_u = chroma ? p.coeff_u : nullptr; a.coeff_v = chroma ? p.coeff_v : nullptr;
    a.cus = (u32 *)p.cus; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
    a.qp = has_lists ? clip_lcu_qp(p.params.qp) : p.params.qp;                  // as the single-picture kernels: clamped with tables only
    a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
    a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
    if (has_lists) { a.quant = r.tables.quant; a.dequant = r.tables.dequant; }
    if (r.ts) { a.lcu_bit_cost = r.ts->lcu_bit_cost; a.tr_skip_out = r.tr_skip_out; a.bit_cost = r.ts->bit_cost; }
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (width >> 2) * (height >> 2));
  }
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(inter_residual_init_multi_ts_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("inter_residual_init_multi_ts_kernel");
  }
  if (lists) {
    launch_pictures<32, true, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<16, true, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<8, true, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    if (skip) launch_pictures<4, true, true>(b, n_pictures, st);
    else launch_pictures<4, true, false>(b, n_pictures, st);
  } else {
    // transform skip with flat lists: the three larger sizes are the kernels of the call without it, on these records
    launch_pictures<32, false, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<16, false, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<8, false, false>(b, n_pictures, st);
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
    launch_pictures<4, false, true>(b, n_pictures, st);
  }
  KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

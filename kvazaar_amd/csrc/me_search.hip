// me_search.hip -- the batched motion search: one launch per size class over a list of PUs (kvz_hip_search_pu_batch,
// kvz_hip_search_pu_multi_batch).  The search itself is me_search_core.h.
#include "me_search_core.h"

using namespace kvzhip;

namespace {

// kvz_hip_search_pu_multi_batch: several pictures of one size in a launch (frames in flight, tiles' or instances' pictures).
// The `pic` / `ref.p` arguments are then DEVICE TABLES of plane pointers, a PU names its pair in pad >> 2, the table length
// travels in prm.n_cabac (unused without mv_rdo).  A template flag, so that the one-picture kernels compile exactly as before.
template <bool MULTI>
__device__ __forceinline__ bool pick_planes(const u8 *__restrict__ &pic, refplane_t &ref, const kvz_hip_me_pu &pu, int n_planes)
{
  if (!MULTI) return true;
  const int k = pu.pad >> 2;
  if (k < 0 || k >= n_planes) return false;
  pic = reinterpret_cast<const u8 *const *>(pic)[k];
  ref.p = reinterpret_cast<const u8 *const *>(ref.p)[k];
  return true;
}

// PUs larger than 32x32 in either direction (and malformed descriptors, which are flagged): one workgroup (T threads) per PU
template <int T, bool CONSTR, bool MULTI = false>
__global__ __launch_bounds__(T) void search_pu_big_kernel(const u8 *__restrict__ pic, u32 pic_stride, int pic_w, int pic_h, refplane_t ref,
                                                            const kvz_hip_me_pu *__restrict__ pus, kvz_hip_me_params prm,
                                                            kvz_hip_me_result *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) u8 lds[frac_geom<64>::TOTAL];
  __shared__ me_shared sh;
  const kvz_hip_me_pu &pu = pus[blockIdx.x];            // uniform address: the compiler reads it with scalar loads
  if (!pu_ok(pu, pic_w, pic_h) || !pick_planes<MULTI>(pic, ref, pu, prm.n_cabac)) { if (threadIdx.x == 0) flag_bad(out + blockIdx.x); return; }
  const int cls = pu_class(pu);
  if (cls != 4) {                                       // the one-wave-per-PU kernels'
    if (pu_orphan(cls, 4, prm.size_classes) && threadIdx.x == 0) flag_bad(out + blockIdx.x);
    return;
  }
  search_pu_core<64, T, false, 0, 0, false, CONSTR>(threadIdx.x, lds, &sh, pic, pic_stride, ref, pu, prm, out + blockIdx.x, blockIdx.x);
}

// --mv-rdo (cfg.mv_rdo, off in every preset): MV bits from the CABAC model.  One workgroup per PU for every size -- a
// correctness path; the model walks probability tables per candidate and is kept out of the kernels above so that their
// register budget is untouched.
__global__ __launch_bounds__(256) void search_pu_rdo_kernel(const u8 *__restrict__ pic, u32 pic_stride, int pic_w, int pic_h, refplane_t ref,
                                                            const kvz_hip_me_pu *__restrict__ pus, kvz_hip_me_params prm,
                                                            kvz_hip_me_result *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) u8 lds[frac_geom<64>::TOTAL];
  __shared__ me_shared sh;
  const kvz_hip_me_pu &pu = pus[blockIdx.x];
  if (!pu_ok(pu, pic_w, pic_h) || pu.reserved < 0 || pu.reserved >= prm.n_cabac) { if (threadIdx.x == 0) flag_bad(out + blockIdx.x); return; }   // a stale snapshot index is flagged, never dereferenced
  search_pu_core<64, 256, false, 0, 0, true>(threadIdx.x, lds, &sh, pic, pic_stride, ref, pu, prm, out + blockIdx.x, blockIdx.x);
}

// PUs up to 16x16: one wave per PU, four PUs per workgroup, wave-private LDS, no barrier.  The register budget is held at
// 6 waves per SIMD (80 VGPRs): at 82 the kernel dropped to 5 and lost 8 % (measured A/B on one box).
template <bool CONSTR, bool MULTI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void search_pu_small_kernel(const u8 *__restrict__ pic, u32 pic_stride, int pic_w, int pic_h, refplane_t ref,
                                                              const kvz_hip_me_pu *__restrict__ pus, size_t count, kvz_hip_me_params prm,
                                                              kvz_hip_me_result *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) u8 lds[4][(frac_geom<16>::TOTAL + 15) & ~15];
  __shared__ me_shared sh[4];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t i = (size_t)blockIdx.x * 4 + wv;
  if (i >= count) return;
  const kvz_hip_me_pu &pu = pus[i];
  const int lane = threadIdx.x & 63;
  if (!pu_ok(pu, pic_w, pic_h) || !pick_planes<MULTI>(pic, ref, pu, prm.n_cabac)) { if (lane == 0) flag_bad(out + i); return; }
  const int cls = pu_class(pu);
  if (cls != 1) {
    if (pu_orphan(cls, 1, prm.size_classes) && lane == 0) flag_bad(out + i);
    return;
  }
  if (pu.width == 8 && pu.height == 8) search_pu_core<16, 64, true, 8, 8, false, CONSTR>(lane, lds[wv], &sh[wv], pic, pic_stride, ref, pu, prm, out + i, i);
  else if (pu.width == 16 && pu.height == 16) search_pu_core<16, 64, true, 16, 16, false, CONSTR>(lane, lds[wv], &sh[wv], pic, pic_stride, ref, pu, prm, out + i, i);
  else search_pu_core<16, 64, true, 0, 0, false, CONSTR>(lane, lds[wv], &sh[wv], pic, pic_stride, ref, pu, prm, out + i, i);
}

// The same class with one workgroup of T threads per PU: lower latency per search (more lanes on each step, barriers
// instead of wave-local fences), lower throughput -- for batches too small to fill the chip with one wave per PU.
template <int T, bool CONSTR, bool MULTI = false>
__global__ __launch_bounds__(T) void search_pu_medium_wg_kernel(const u8 *__restrict__ pic, u32 pic_stride, int pic_w, int pic_h, refplane_t ref,
                                                                const kvz_hip_me_pu *__restrict__ pus, kvz_hip_me_params prm,
                                                                kvz_hip_me_result *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) u8 lds[(frac_geom<32>::TOTAL + 15) & ~15];
  __shared__ me_shared sh;
  const kvz_hip_me_pu &pu = pus[blockIdx.x];
  if (!pu_ok(pu, pic_w, pic_h) || !pick_planes<MULTI>(pic, ref, pu, prm.n_cabac)) { if (threadIdx.x == 0) flag_bad(out + blockIdx.x); return; }
  const int cls = pu_class(pu);
  if (cls != 2) {
    if (pu_orphan(cls, 2, prm.size_classes) && threadIdx.x == 0) flag_bad(out + blockIdx.x);
    return;
  }
  if (pu.width == 32 && pu.height == 32) search_pu_core<32, T, false, 32, 32, false, CONSTR>(threadIdx.x, lds, &sh, pic, pic_stride, ref, pu, prm, out + blockIdx.x, blockIdx.x);
  else search_pu_core<32, T, false, 0, 0, false, CONSTR>(threadIdx.x, lds, &sh, pic, pic_stride, ref, pu, prm, out + blockIdx.x, blockIdx.x);
}

}  // namespace

template <bool CONSTR, bool MULTI>
static void launch_classes(int classes, const u8 *pic, u32 pic_stride, int pic_w, int pic_h, const refplane_t &r, const kvz_hip_me_pu *pus,
                           size_t count, const kvz_hip_me_params &prm, kvz_hip_me_result *results, hipStream_t st)
{
  // one launch per size class over the same descriptor list; each kernel takes its class and skips the rest
  if (classes == 7 || (classes & 4))
    hipLaunchKernelGGL((search_pu_big_kernel<512, CONSTR, MULTI>), dim3((unsigned)count), dim3(512), 0, st, pic, pic_stride, pic_w, pic_h, r, pus, prm, results);
  if (classes & 1)
    hipLaunchKernelGGL((search_pu_small_kernel<CONSTR, MULTI>), dim3((unsigned)((count + 3) / 4)), dim3(256), 0, st, pic, pic_stride, pic_w, pic_h, r, pus, count, prm, results);
  if (classes & 2)
    hipLaunchKernelGGL((search_pu_medium_wg_kernel<128, CONSTR, MULTI>), dim3((unsigned)count), dim3(128), 0, st, pic, pic_stride, pic_w, pic_h, r, pus, prm, results);
}

// n_planes == 0: pic / ref are the planes; > 0: device tables of that many plane pointers (kvz_hip_search_pu_multi_batch)
static int search_pu_launch(const kvz_hip_pixel *pic, uint32_t pic_stride, int pic_w, int pic_h,
                            const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h, int n_planes,
                            const kvz_hip_me_pu *pus, size_t count, const kvz_hip_me_params *params,
                            kvz_hip_me_result *results, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!pic || !ref || !pus || !params || !results || pic_w <= 0 || pic_h <= 0 || ref_w <= 0 || ref_h <= 0) {
    set_error_msg("kvz_hip_search_pu_batch: null buffer or empty plane");
    return KVZ_HIP_ERR_INVALID;
  }
  if (params->lambda_cost < 0 || params->lambda_cost > (1 << 20)) {
    set_error_msg("kvz_hip_search_pu_batch: lambda_cost must be within 0 .. 2^20 (costs are 32-bit like the reference's)");
    return KVZ_HIP_ERR_INVALID;
  }
  if (params->fme_level < 0 || params->fme_level > 4 || params->early_termination < 0 || params->early_termination > 2 ||
      params->algorithm < 0 || params->algorithm > 3 ||
      (params->algorithm == 3 && (params->search_range < 1 || params->search_range > 64))) {
    set_error_msg("kvz_hip_search_pu_batch: fme_level must be 0..4, early_termination 0..2, algorithm 0 (hexbs), 1 (dia), 2 (tz) or 3 (full, search_range 1..64)");
    return KVZ_HIP_ERR_INVALID;
  }
  kvz_hip_me_params prm_v = *params;
  if (prm_v.tile_w == 0 && prm_v.tile_h == 0) { prm_v.tile_x = 0; prm_v.tile_y = 0; prm_v.tile_w = pic_w; prm_v.tile_h = pic_h; }
  if (prm_v.mv_constraint < 0 || prm_v.mv_constraint > 4 || prm_v.tile_x < 0 || prm_v.tile_y < 0 || prm_v.tile_w <= 0 || prm_v.tile_h <= 0 ||
      prm_v.tile_x + prm_v.tile_w > pic_w || prm_v.tile_y + prm_v.tile_h > pic_h || (prm_v.wpp_owf && ((prm_v.tile_x & 63) || (prm_v.tile_y & 63)))) {
    set_error_msg("kvz_hip_search_pu_batch: mv_constraint must be 0..4 and the tile must lie inside the picture (origin a multiple of 64 when wpp_owf is set: its rule counts LCUs from there)");
    return KVZ_HIP_ERR_INVALID;
  }
  params = &prm_v;
  if (count == 0) return KVZ_HIP_OK;
  if (count > 0x7fffffffu) return kvzhip::invalid_arg(__func__);
  hipStream_t st = ctx_stream(s);
  const refplane_t r = { ref, ref_stride, ref_w, ref_h };
  // one launch per size class over the same descriptor list; each kernel takes its class and skips the rest.  The big
  // kernel also flags malformed descriptors, so it only goes when the caller vouches for the classes it names.
  if (params->mv_rdo) {
    if (n_planes) { set_error_msg("kvz_hip_search_pu_multi_batch: mv_rdo is a one-picture path"); return KVZ_HIP_ERR_INVALID; }
    if (!params->cabac || params->n_cabac < 1 || params->refs_before < 1 || params->refs_before > 16 || params->ref_idx < 0 || params->ref_idx >= 16) {
      set_error_msg("kvz_hip_search_pu_batch: mv_rdo needs the cabac snapshots (device array of n_cabac >= 1), refs_before 1..16 and ref_idx 0..15");
      return KVZ_HIP_ERR_INVALID;
    }
    hipLaunchKernelGGL(search_pu_rdo_kernel, dim3((unsigned)count), dim3(256), 0, st, pic, pic_stride, pic_w, pic_h, r, pus, *params, results);
    KVZ_CHECK_LAUNCH("search_pu_rdo_kernel");
    return KVZ_HIP_OK;
  }
  // with a hint, PUs of a class it does not name are searched by no kernel: they read cost 0xFFFFFFFF, reserved -1
  // (pu_orphan: written by the kernels themselves -- a separate fill would be one more command per dependency front)
  const int classes = (params->size_classes & 7) ? (params->size_classes & 7) : 7;
  prm_v.size_classes = classes;
  prm_v.n_cabac = n_planes;                             // the multi-picture kernels find the table length here (mv_rdo is a one-picture path)
  // thread counts are measured choices: > 32x32: 512 threads per PU 10.5 M/s (256: 9.5, 1024: 6.5); <= 32x32: 128 per PU 48.9 M/s
  // (256: 46.6, one wave: 42.6); <= 16x16: one wave per PU, four per workgroup
  const bool constrained = params->wpp_owf != 0 || params->mv_constraint != 0;
  if (n_planes) {
    if (constrained) launch_classes<true, true>(classes, pic, pic_stride, pic_w, pic_h, r, pus, count, *params, results, st);
    else launch_classes<false, true>(classes, pic, pic_stride, pic_w, pic_h, r, pus, count, *params, results, st);
  } else {
    if (constrained) launch_classes<true, false>(classes, pic, pic_stride, pic_w, pic_h, r, pus, count, *params, results, st);
    else launch_classes<false, false>(classes, pic, pic_stride, pic_w, pic_h, r, pus, count, *params, results, st);
  }
  KVZ_CHECK_LAUNCH("search_pu kernels");
  return KVZ_HIP_OK;
}

extern "C" int kvz_hip_search_pu_batch(const kvz_hip_pixel *pic, uint32_t pic_stride, int pic_w, int pic_h,
                                       const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                       const kvz_hip_me_pu *pus, size_t count, const kvz_hip_me_params *params,
                                       kvz_hip_me_result *results, kvz_hip_stream s)
{
  return search_pu_launch(pic, pic_stride, pic_w, pic_h, ref, ref_stride, ref_w, ref_h, 0, pus, count, params, results, s);
}

extern "C" int kvz_hip_search_pu_multi_batch(const kvz_hip_pixel *const *pics, uint32_t pic_stride, int pic_w, int pic_h,
                                             const kvz_hip_pixel *const *refs, uint32_t ref_stride, int ref_w, int ref_h, int n_planes,
                                             const kvz_hip_me_pu *pus, size_t count, const kvz_hip_me_params *params,
                                             kvz_hip_me_result *results, kvz_hip_stream s)
{
  if (n_planes < 1 || n_planes > 8192) { set_error_msg("kvz_hip_search_pu_multi_batch: 1 .. 8192 plane pairs"); return KVZ_HIP_ERR_INVALID; }
  return search_pu_launch(reinterpret_cast<const kvz_hip_pixel *>(pics), pic_stride, pic_w, pic_h, reinterpret_cast<const kvz_hip_pixel *>(refs),
                          ref_stride, ref_w, ref_h, n_planes, pus, count, params, results, s);
}

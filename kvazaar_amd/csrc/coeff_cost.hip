// coeff_cost.hip -- kvz_hip_coeff_cost_batch: the reference's CABAC price (get_coeff_cabac_cost, rdo.c:158-197) of a list of TUs that lie
// in device memory, each from one of the caller's context sets (coeff_cabac_core.h holds the counter).
// Two launches over the same descriptor list, each taking the descriptors of its class and passing over the others:
//   small: a lane per 4x4 TU.  The lane keeps its 16 coefficients and its private copy of the context set in the wave's LDS,
//          lane-interleaved, because the counter indexes both with computed values.
//   large: a wave per TU of width 8 / 16 / 32.  The wave stages the TU and the set in LDS once with row-contiguous loads, finds
//          the coefficient groups that hold something with one ballot, and one lane runs the serial recursion.
// Only the (range, context state) recursion is serial; a later change can hand the large kernel's idle lanes the bin derivation.
#include "coeff_cabac_core.h"
#include "coeff_cost_host.h"

#include <stdio.h>

static_assert(kvzhip::CC_CTX_USED % 2 == 0 && offsetof(kvz_hip_coeff_ctx, ctx) % 2 == 0, "the small kernel copies a set in byte pairs");

namespace kvzhip {

// what a descriptor must satisfy to be priced at all; everything the kernels index with is bounded by it
__device__ __forceinline__ bool cc_desc_ok(const kvz_hip_coeff_cost_desc &d, u32 n_sets)
{
  const bool width_ok = d.width == 4 || d.width == 8 || d.width == 16 || d.width == 32;
  return width_ok && (d.type == 0 || d.type == 2) && (d.scan_mode == 0 || (d.scan_mode <= 2 && d.width <= 8)) && d.tr_skip <= 1 &&
         (d.offset & 3u) == 0 && d.ctx_index < n_sets;
}

// the context set and the coefficients of lane `lane`'s TU, interleaved over the wave's 64 lanes
struct cc_lane_ctx {
  u8 *p;
  __device__ __forceinline__ u32 get(int i) const { return p[i * 64]; }
  __device__ __forceinline__ void set(int i, u32 v) { p[i * 64] = (u8)v; }
};
struct cc_lane_coeffs {
  const u32 *p;                                                // dword k of the TU at p[k * 64]
  __device__ __forceinline__ int at(int x, int y) const
  {
    const u32 w = p[(2 * y + (x >> 1)) * 64];
    return (int)(i16)(x & 1 ? w >> 16 : w & 0xffffu);
  }
};
// the one TU of a wave, row-major
struct cc_wave_ctx {
  u8 *p;
  __device__ __forceinline__ u32 get(int i) const { return p[i]; }
  __device__ __forceinline__ void set(int i, u32 v) { p[i] = (u8)v; }
};
struct cc_wave_coeffs {
  const i16 *p;
  int log2w;
  __device__ __forceinline__ int at(int x, int y) const { return p[(y << log2w) + x]; }
};

__device__ __forceinline__ coeff_cabac_flags cc_flags(const kvz_hip_coeff_cost_params &prm)
{
  return { prm.signhide != 0, prm.trskip_enable != 0, prm.lossless != 0 };
}

__global__ void __launch_bounds__(64) coeff_cost_small_kernel(const kvz_hip_coeff *__restrict__ coeffs, const kvz_hip_coeff_cost_desc *__restrict__ descs, u32 n,
                                                              const kvz_hip_coeff_ctx *__restrict__ ctx_sets, u32 n_sets, kvz_hip_coeff_cost_params prm,
                                                              u32 *__restrict__ bits_out)
{
  __shared__ u32 s_coeffs[8 * 64];
  __shared__ u8 s_ctx[CC_CTX_USED * 64];
  const u32 lane = threadIdx.x, i = blockIdx.x * 64u + lane;
  if (i >= n) return;
  const kvz_hip_coeff_cost_desc d = descs[i];
  if (!cc_desc_ok(d, n_sets) || d.width != 4) return;
  const uint2 *src = (const uint2 *)(coeffs + d.offset);       // offset % 4 == 0 on an 8-byte aligned array
  u32 any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint2 v = src[k];
    s_coeffs[(2 * k) * 64 + lane] = v.x;
    s_coeffs[(2 * k + 1) * 64 + lane] = v.y;
    any |= v.x | v.y;
  }
  u32 bits = 0;
  if (any) {
    const kvz_hip_coeff_ctx &set = ctx_sets[d.ctx_index];
    const uint16_t *pairs = (const uint16_t *)set.ctx;          // a set is 2-byte aligned and ctx lies at offset 4: two bytes a load
    for (int k = 0; k < CC_CTX_USED / 2; ++k) {
      const u32 v = pairs[k];
      s_ctx[(2 * k) * 64 + lane] = (u8)v;
      s_ctx[(2 * k + 1) * 64 + lane] = (u8)(v >> 8);
    }
    const cc_lane_coeffs cf = { s_coeffs + lane };
    const cc_lane_ctx ctx = { s_ctx + lane };
    bits = coeff_cabac_count(cf, ctx, set.range, 2, d.type, d.scan_mode, d.tr_skip, cc_flags(prm), 1ull);
  }
  bits_out[i] = bits;
}

__global__ void __launch_bounds__(64) coeff_cost_large_kernel(const kvz_hip_coeff *__restrict__ coeffs, const kvz_hip_coeff_cost_desc *__restrict__ descs, u32 n,
                                                              const kvz_hip_coeff_ctx *__restrict__ ctx_sets, u32 n_sets, kvz_hip_coeff_cost_params prm,
                                                              u32 *__restrict__ bits_out)
{
  __shared__ uint2 s_coeffs[32 * 32 / 4];
  __shared__ u8 s_ctx[CC_CTX_USED + 2];
  const u32 lane = threadIdx.x;
  for (u32 i = blockIdx.x; i < n; i += gridDim.x) {            // i is the same in every lane: no lane leaves the wave's fences alone
    const kvz_hip_coeff_cost_desc d = descs[i];
    if (!cc_desc_ok(d, n_sets) || d.width == 4) continue;
    const int log2w = d.width == 8 ? 3 : d.width == 16 ? 4 : 5, quads = (d.width * d.width) >> 2, g = d.width >> 2;
    const uint2 *src = (const uint2 *)(coeffs + d.offset);
    wave_lds_fence();                                          // the previous TU's reads are done
    for (int k = (int)lane; k < quads; k += 64) s_coeffs[k] = src[k];
    const kvz_hip_coeff_ctx &set = ctx_sets[d.ctx_index];
    for (int k = (int)lane; k < CC_CTX_USED; k += 64) s_ctx[k] = set.ctx[k];
    wave_lds_fence();
    // lane = group x + y * g: four rows of one quad each
    bool has = false;
    if ((int)lane < g * g) {
      const int qx = (int)lane & (g - 1), qy = (int)lane >> (log2w - 2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint2 v = s_coeffs[(qy * 4 + r) * g + qx];
        has = has || (v.x | v.y) != 0;
      }
    }
    const unsigned long long sig_cg = __ballot(has);
    if (lane == 0) {
      const cc_wave_coeffs cf = { (const i16 *)s_coeffs, log2w };
      const cc_wave_ctx ctx = { s_ctx };
      bits_out[i] = coeff_cabac_count(cf, ctx, set.range, log2w, d.type, d.scan_mode, d.tr_skip, cc_flags(prm), sig_cg);
    }
  }
}

}  // namespace kvzhip

extern "C" {

int kvz_hip_coeff_cost_batch(const kvz_hip_coeff *coeffs, const kvz_hip_coeff_cost_desc *descs, size_t n, const kvz_hip_coeff_ctx *ctx_sets,
                             uint32_t n_sets, const kvz_hip_coeff_cost_params *params, uint32_t *bits_out, kvz_hip_stream s)
{
  using namespace kvzhip;
  KVZ_CHECK_CTX();
  if (n == 0) return KVZ_HIP_OK;
  if (const char *why = coeff_cost_batch_why(coeffs, descs, n, ctx_sets, n_sets, params, bits_out)) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: invalid argument (%s)", __func__, why);
    set_error_msg(msg);
    return KVZ_HIP_ERR_INVALID;
  }
  hipStream_t st = ctx_stream(s);
  const u32 count = (u32)n;
  hipLaunchKernelGGL(coeff_cost_small_kernel, dim3((count + 63) / 64), dim3(64), 0, st, coeffs, descs, count, ctx_sets, n_sets, *params, bits_out);
  KVZ_CHECK_LAUNCH("coeff_cost_small_kernel");
  hipLaunchKernelGGL(coeff_cost_large_kernel, dim3(stream_grid(count, 1, 32)), dim3(64), 0, st, coeffs, descs, count, ctx_sets, n_sets, *params, bits_out);
  KVZ_CHECK_LAUNCH("coeff_cost_large_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

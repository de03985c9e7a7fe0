// rdoq.hip -- kvz_hip_rdoq_batch: the reference's kvz_rdoq (rdo.c:548-881) over a list of TUs that lie in device memory, each with
// the contexts, lambda and QP of one of the caller's records (rdoq_core.h holds the arithmetic), and kvz_hip_rdoq_tables_pack.
// Two launches over the same descriptor list, each taking the descriptors of its class and passing over the others, as
// coeff_cost.hip does:
//   small: a lane per 4x4 TU.  Every array of the recursion lies in the wave's LDS, lane-interleaved.
//   large: a wave per TU of width 8 / 16 / 32.  The wave stages the TU, the context set and the state in LDS; level_double and
//          err * err * temp are computed across the lanes, a ballot finds last_scanpos, lane 0 runs the serial recursion, the signs
//          and the clean-up go across the lanes again, and sign hiding runs with a lane per coefficient group.
// A first structure: the recursion of one TU keeps one lane busy and its arrays take about 50 KB of LDS per wave, which holds the
// large kernel to three waves per CU.
#include "rdoq_core.h"
#include "quant_core.h"
#include "rdoq_stage.h"
#include "rdoq_host.h"

#include <stdio.h>

#pragma clang fp contract(off)

static_assert(offsetof(kvz_hip_coeff_ctx, ctx) == 4, "layout documented in kvz_hip.h");

namespace kvzhip {

// what a descriptor must satisfy to be quantised at all; everything the kernels index with is bounded by it and by rdoq_state_ok
__device__ __forceinline__ bool rdoq_desc_ok(const kvz_hip_rdoq_desc &d, u32 n_sets)
{
  const bool width_ok = d.width == 4 || d.width == 8 || d.width == 16 || d.width == 32;
  return width_ok && (d.type == 0 || d.type == 2) && (d.scan_mode == 0 || (d.scan_mode <= 2 && d.width <= 8)) &&
         (d.block_type == 1 || d.block_type == 2) && d.tr_depth <= 3 && (d.src_offset & 3u) == 0 && (d.dst_offset & 3u) == 0 && d.ctx_index < n_sets;
}
__device__ __forceinline__ bool rdoq_qp_ok(int qp) { return qp >= 0 && qp <= 51; }

__global__ void __launch_bounds__(64) rdoq_small_kernel(const kvz_hip_coeff *__restrict__ coef, kvz_hip_coeff *__restrict__ dest,
                                                        const kvz_hip_rdoq_desc *__restrict__ descs, u32 n, const kvz_hip_coeff_ctx *__restrict__ ctx_sets,
                                                        const kvz_hip_rdoq_state *__restrict__ states, u32 n_sets, kvz_hip_rdoq_tables tables, int signhide)
{
  __shared__ double s_c0[16 * 64], s_cc[16 * 64], s_cs[16 * 64], s_cg[64];
  __shared__ i32 s_ld[16 * 64], s_sig[16 * 64], s_inc[16 * 64], s_dec[16 * 64], s_qd[16 * 64], s_lx[4 * 64], s_ly[4 * 64];
  __shared__ i16 s_dst[16 * 64], s_coef[16 * 64];
  const u32 lane = threadIdx.x, i = blockIdx.x * 64u + lane;
  if (i >= n) return;
  const kvz_hip_rdoq_desc d = descs[i];
  if (!rdoq_desc_ok(d, n_sets) || d.width != 4) return;
  const kvz_hip_rdoq_state &st = states[d.ctx_index];
  const int qp = st.qp;
  if (!rdoq_qp_ok(qp)) return;
  int table_at;
  const rdoq_tu t = rdoq_make_tu(d, qp, st.lambda, signhide, table_at);
  const i32 *quant = tables.quant + table_at;
  const double *err_scale = tables.err_scale + table_at;
  const rdoq_mem<64> m = { s_c0 + lane, s_cc + lane, s_cs + lane, s_cg + lane, s_ld + lane, s_sig + lane, s_inc + lane, s_dec + lane, s_qd + lane,
                           s_lx + lane, s_ly + lane, s_dst + lane, s_coef + lane };
  u8 state_ctx[RQ_STATE_CTX];
#pragma unroll
  for (int k = 0; k < RQ_STATE_CTX; ++k) state_ctx[k] = rdoq_state_byte(st, k);
  const rdoq_ctx ctx = { ctx_sets[d.ctx_index].ctx, state_ctx };
  const rdoq_scan sc = rdoq_make_scan(2, d.scan_mode);

  const uint2 *src = (const uint2 *)(coef + d.src_offset);       // src_offset % 4 == 0 on an 8-byte aligned array
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint2 v = src[k];
    s_coef[(4 * k) * 64 + lane] = (i16)(v.x & 0xffffu);
    s_coef[(4 * k + 1) * 64 + lane] = (i16)(v.x >> 16);
    s_coef[(4 * k + 2) * 64 + lane] = (i16)(v.y & 0xffffu);
    s_coef[(4 * k + 3) * 64 + lane] = (i16)(v.y >> 16);
  }
  int last_scanpos = -1;
  for (int s = 0; s < 16; ++s) {
    const int blk = sc.blk(s);
    if (rdoq_prepare(m, blk, quant[blk], err_scale[blk], t.q_bits) > 0) last_scanpos = s;
  }
  int best = 0;
  if (last_scanpos >= 0) best = rdoq_recursion(m, ctx, sc, t, err_scale, last_scanpos);
  u32 abs_sum = 0;
  for (int s = 0; s < 16; ++s) abs_sum += rdoq_finish(m, sc.blk(s), s, best);
  if (t.signhide && abs_sum >= 2) rdoq_sign_hide_group(m, sc, 0, 0, rdoq_rd_factor(t.qp_scaled, t.lambda));
  uint2 *out = (uint2 *)(dest + d.dst_offset);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint2 v;
    v.x = (u32)(uint16_t)s_dst[(4 * k) * 64 + lane] | (u32)(uint16_t)s_dst[(4 * k + 1) * 64 + lane] << 16;
    v.y = (u32)(uint16_t)s_dst[(4 * k + 2) * 64 + lane] | (u32)(uint16_t)s_dst[(4 * k + 3) * 64 + lane] << 16;
    out[k] = v;
  }
}

__global__ void __launch_bounds__(64) rdoq_large_kernel(const kvz_hip_coeff *__restrict__ coef, kvz_hip_coeff *__restrict__ dest,
                                                        const kvz_hip_rdoq_desc *__restrict__ descs, u32 n, const kvz_hip_coeff_ctx *__restrict__ ctx_sets,
                                                        const kvz_hip_rdoq_state *__restrict__ states, u32 n_sets, kvz_hip_rdoq_tables tables, int signhide)
{
  __shared__ double s_c0[1024], s_cc[1024], s_cs[1024], s_cg[64];
  __shared__ i32 s_ld[1024], s_sig[1024], s_inc[1024], s_dec[1024], s_qd[1024], s_lx[12], s_ly[12];
  __shared__ alignas(8) i16 s_dst[1024], s_coef[1024];           // moved to and from global memory eight bytes at a time, by memcpy: one type per array
  __shared__ u8 s_ctx[CC_CTX_USED + 2], s_state[RQ_STATE_CTX + 3];
  const u32 lane = threadIdx.x;
  const rdoq_mem<1> m = { s_c0, s_cc, s_cs, s_cg, s_ld, s_sig, s_inc, s_dec, s_qd, s_lx, s_ly, s_dst, s_coef };
  const rdoq_ctx ctx = { s_ctx, s_state };
  for (u32 i = blockIdx.x; i < n; i += gridDim.x) {              // i is the same in every lane: no lane leaves the wave's fences alone
    const kvz_hip_rdoq_desc d = descs[i];
    if (!rdoq_desc_ok(d, n_sets) || d.width == 4) continue;
    const kvz_hip_rdoq_state &st = states[d.ctx_index];
    const int qp = st.qp;
    if (!rdoq_qp_ok(qp)) continue;
    int table_at;
    const rdoq_tu t = rdoq_make_tu(d, qp, st.lambda, signhide, table_at);
    const i32 *quant = tables.quant + table_at;
    const double *err_scale = tables.err_scale + table_at;
    const rdoq_scan sc = rdoq_make_scan(t.log2w, d.scan_mode);
    const int n2 = d.width * d.width, quads = n2 >> 2;
    const uint2 *src = (const uint2 *)(coef + d.src_offset);
    wave_lds_fence();                                              // the previous TU's reads are done
    for (int k = (int)lane; k < quads; k += 64) {
      const uint2 v = src[k];
      __builtin_memcpy(&s_coef[4 * k], &v, sizeof v);
    }
    const kvz_hip_coeff_ctx &set = ctx_sets[d.ctx_index];
    for (int k = (int)lane; k < CC_CTX_USED - 2; k += 64) s_ctx[k] = set.ctx[k];
    if (lane < RQ_STATE_CTX) s_state[lane] = rdoq_state_byte(st, (int)lane);
    wave_lds_fence();
    // per scan position: level_double, cost_coeff0, and the last position whose max_abs_level is above 0 (rdo.c:621-642)
    int last_scanpos = -1;
    for (int s0 = 0; s0 < n2; s0 += 64) {
      const int blk = sc.blk(s0 + (int)lane);
      const bool some = rdoq_prepare(m, blk, quant[blk], err_scale[blk], t.q_bits) > 0;
      const unsigned long long mask = __ballot(some);
      if (mask) last_scanpos = s0 + 63 - __clzll((long long)mask);
    }
    wave_lds_fence();
    int best = 0;
    if (last_scanpos >= 0) {
      if (lane == 0) best = rdoq_recursion(m, ctx, sc, t, err_scale, last_scanpos);
      best = __builtin_amdgcn_readfirstlane(best);
      wave_lds_fence();
    }
    // signs and clean-up (rdo.c:866-876); abs_sum matters only as "at least 2"
    u32 abs_sum = 0;
    for (int s0 = 0; s0 < n2; s0 += 64) {
      const int s = s0 + (int)lane;
      const u32 level = rdoq_finish(m, sc.blk(s), s, best);
      abs_sum += level > 2 ? 2 : level;
    }
    const unsigned long long ones = __ballot(abs_sum == 1), more = __ballot(abs_sum >= 2);
    wave_lds_fence();
    if (t.signhide && (more || __popcll(ones) >= 2)) {
      const int last_cg = (best - 1) >> 4;
      if ((int)lane <= last_cg) rdoq_sign_hide_group(m, sc, (int)lane, last_cg, rdoq_rd_factor(t.qp_scaled, t.lambda));
      wave_lds_fence();
    }
    uint2 *out = (uint2 *)(dest + d.dst_offset);
    for (int k = (int)lane; k < quads; k += 64) {
      uint2 v;
      __builtin_memcpy(&v, &s_dst[4 * k], sizeof v);
      out[k] = v;
    }
  }
}

}  // namespace kvzhip

extern "C" {

int kvz_hip_rdoq_tables_pack(const int32_t *const quant_coeff[4][6][6], const double *const error_scale[4][6][6], int32_t *quant_out, double *err_out)
{
  if (!quant_coeff || !error_scale || !quant_out || !err_out) return kvzhip::invalid_arg(__func__);
  // the 32x32 lists the reference holds are [3][0], [3][1] and [3][3], a second name of [3][1] (see kvz_hip_scaling_tables_pack)
  auto held = [](int size_id, int list) { return size_id < 3 || list == 0 || list == 1 || list == 3; };
  for (int size_id = 0; size_id < 4; ++size_id)
    for (int list = 0; list < 6; ++list)
      for (int rem = 0; rem < 6; ++rem)
        if (held(size_id, list) && (!quant_coeff[size_id][list][rem] || !error_scale[size_id][list][rem])) return kvzhip::invalid_arg(__func__);
  for (int size_id = 0; size_id < 4; ++size_id) {
    const size_t count = (size_t)16 << (2 * size_id);
    for (int list = 0; list < 6; ++list) {
      for (int rem = 0; rem < 6; ++rem) {
        const int at = sl_table_offset(size_id, list, rem);
        if (held(size_id, list)) {
          __builtin_memcpy(quant_out + at, quant_coeff[size_id][list][rem], count * sizeof(int32_t));
          __builtin_memcpy(err_out + at, error_scale[size_id][list][rem], count * sizeof(double));
        } else {
          __builtin_memset(quant_out + at, 0, count * sizeof(int32_t));
          __builtin_memset(err_out + at, 0, count * sizeof(double));
        }
      }
    }
  }
  return KVZ_HIP_OK;
}

int kvz_hip_rdoq_batch(const kvz_hip_coeff *coef, kvz_hip_coeff *dest, const kvz_hip_rdoq_desc *descs, size_t n, const kvz_hip_coeff_ctx *ctx_sets,
                       const kvz_hip_rdoq_state *states, uint32_t n_sets, const kvz_hip_rdoq_tables *tables, const kvz_hip_rdoq_params *params,
                       kvz_hip_stream s)
{
  using namespace kvzhip;
  KVZ_CHECK_CTX();
  if (n == 0) return KVZ_HIP_OK;
  if (const char *why = rdoq_batch_why(coef, dest, descs, n, ctx_sets, states, n_sets, tables, params)) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: invalid argument (%s)", __func__, why);
    set_error_msg(msg);
    return KVZ_HIP_ERR_INVALID;
  }
  hipStream_t st = ctx_stream(s);
  const u32 count = (u32)n;
  const int signhide = params->signhide != 0;
  hipLaunchKernelGGL(rdoq_small_kernel, dim3((count + 63) / 64), dim3(64), 0, st, coef, dest, descs, count, ctx_sets, states, n_sets, *tables, signhide);
  KVZ_CHECK_LAUNCH("rdoq_small_kernel");
  // about 50 KB of LDS a wave: three workgroups a CU
  hipLaunchKernelGGL(rdoq_large_kernel, dim3(stream_grid(count, 1, 3)), dim3(64), 0, st, coef, dest, descs, count, ctx_sets, states, n_sets, *tables, signhide);
  KVZ_CHECK_LAUNCH("rdoq_large_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

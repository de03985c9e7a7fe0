// sao_stats_core.h -- the kernel of the per-LCU statistics of the whole-picture SAO entries (sao_frame.hip: a picture,
// sao_frame_multi.hip: several pictures).  Everything here has internal linkage: each translation unit gets its own copy and
// instantiates one kernel.  The algorithm is described in sao_frame.hip.
#pragma once

#include "sao_frame_core.h"

namespace {

__device__ __forceinline__ int wave_sum(int v) { return (int)group_sum<64>((u32)v); }

struct stats_args {
  const u8 *src[3], *rec[3];
  u32 src_stride[2], rec_stride[2];       // [0] luma, [1] chroma
  int width, height, lcus_x, n_lcu;
  int *stats, *cands;                     // 104 / 30 int32 per record; cands may be NULL
};
// host: the argument of one picture, for kvz_hip_sao_stats_frame and a record of kvz_hip_sao_stats_frames
inline void sao_stats_fill(stats_args &a, const kvz_hip_filter_picture &p)
{
  const bool chroma = p.chroma != 0;
  a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.src_stride[0] = p.src.stride_y; a.src_stride[1] = p.src.stride_c;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = p.stride_c;
  a.width = p.width; a.height = p.height;
  a.lcus_x = (p.width + 63) >> 6;
  a.n_lcu = a.lcus_x * ((p.height + 63) >> 6);
  a.stats = (int *)p.stats; a.cands = (int *)p.cands;
}

// offset of one category or band: the mean error rounded to nearest with C's truncating division, clipped to SAO_ABS_OFFSET_MAX
// at bit depth 8 (sao.c:205-206, :381-382)
__device__ __forceinline__ int mean_offset(int sum, int cnt)
{
  return cnt ? clampi((sum + (cnt >> 1)) / cnt, -7, 7) : 0;
}

// BATCH: nothing (kvz_hip_sao_stats_frame), or the table of the pictures of a multi-picture call as an optional trailing argument
// (kvz_hip_sao_stats_frames, sao_frame_multi.hip), the picture being the grid's second dimension: the arguments are the record's and
// the kernel's own are not read; a workgroup beyond its picture's LCUs leaves at once.  Without it the instantiation is the kernel as
// it was.
struct stats_batch { stats_args p[KVZ_HIP_MAX_CHAIN_PICTURES]; };
static_assert(sizeof(stats_args) == 96 && sizeof(stats_batch) <= 4096, "the records travel in the kernel arguments");
// a[i] for i = 0, 1 (, 2) with constant indices only, for an `a` that was copied out of the table: selected, not indexed
template <typename T> __device__ __forceinline__ T pick2(const T (&a)[2], int i) { return i ? a[1] : a[0]; }
template <typename T> __device__ __forceinline__ T pick3(const T (&a)[3], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }
__device__ __forceinline__ const stats_batch &only(const stats_batch &b) { return b; }
template <typename... BATCH>
__global__ __launch_bounds__(256) void sao_stats_frame_kernel(stats_args a, BATCH... batch)
{
  constexpr bool BATCHED = sizeof...(BATCH) != 0;
  if constexpr (BATCHED) {
    a = only(batch...).p[blockIdx.y];
    if ((int)blockIdx.x >= a.n_lcu * (a.rec[1] ? 3 : 1)) return;
  }
  __shared__ u32 s_r[64 * 64 / 4];
  __shared__ u32 s_hist[4][32];             // per wave and band: count << 20 | sum of (orig - rec + 255)
  __shared__ int s_out[104];                // the statistics record: edge[4][2][5], band[2][32]
  __shared__ int s_dist[32], s_boff[32];
  __shared__ int s_cand[30];                // the candidate record
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int color = (int)blockIdx.x / a.n_lcu, lcu = (int)blockIdx.x - color * a.n_lcu;
  const int ly = lcu / a.lcus_x, lx = lcu - ly * a.lcus_x;
  const int sh = color ? 1 : 0, bs = 64 >> sh;
  const int pw = a.width >> sh, ph = a.height >> sh;
  const int x0 = lx * bs, y0 = ly * bs;
  const int bw = min(bs, pw - x0), bh = min(bs, ph - y0);      // sao.c:588-601: clipped at the right and bottom picture edge
  const int g4 = bw >> 2, n4 = g4 * bh;
  u32 rs, os;
  const u8 *rec, *org;
  if constexpr (BATCHED) {
    rs = pick2(a.rec_stride, sh); os = pick2(a.src_stride, sh);
    rec = pick3(a.rec, color) + (size_t)y0 * rs + x0;
    org = pick3(a.src, color) + (size_t)y0 * os + x0;
  } else {
    rs = a.rec_stride[sh]; os = a.src_stride[sh];
    rec = a.rec[color] + (size_t)y0 * rs + x0;
    org = a.src[color] + (size_t)y0 * os + x0;
  }
  const u32 recip = (65536u + (u32)g4 - 1u) / (u32)g4;         // it / g4 == (it * recip) >> 16 for it < 1024, g4 <= 16

  for (int i = tid; i < n4; i += 256) {
    const int y = (int)(((u32)i * recip) >> 16), xg = i - y * g4;
    s_r[i] = *(const u32 *)(rec + (size_t)y * rs + 4 * xg);
  }
  if (tid < 128) (&s_hist[0][0])[tid] = 0;
  if (tid < 40) s_out[tid] = 0;
  __syncthreads();

  // a lane sees at most 4 items = 16 pixels: counts fit 7-bit fields, sums of (diff + 255) 15-bit fields
  unsigned long long sum[4] = { 0, 0, 0, 0 };
  u32 cnt[4] = { 0, 0, 0, 0 };
  int tot = 0, npx = 0;
  for (int it = tid; it < n4; it += 256) {
    const int y = (int)(((u32)it * recip) >> 16), xg = it - y * g4;
    const u32 cd = s_r[it], od = *(const u32 *)(org + (size_t)y * os + 4 * xg);
    // calc_sao_bands: every pixel of the block; bit depth 8, so the band is rec >> 3
    {
      int pb = (int)(cd & 255u) >> 3;
      u32 pv = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rv = (int)((cd >> (8 * k)) & 255u), ov = (int)((od >> (8 * k)) & 255u), b = rv >> 3;
        const u32 v = (1u << 20) + (u32)(ov - rv + 255);
        if (b != pb) { atomicAdd(&s_hist[wv][pb], pv); pb = b; pv = 0; }
        pv += v;
      }
      atomicAdd(&s_hist[wv][pb], pv);
    }
    if (y < 1 || y > bh - 2) continue;       // calc_sao_edge_dir: the interior only
    // rows y-1, y, y+1 as 6-pixel windows: [last byte of the left dword, the dword, first byte of the right dword]
    int win[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // the outer neighbour dword of a row's first / last item belongs to another row or lies outside the block: those pixels
      // are excluded border columns, any value will do, but the read stays inside the array
      const int il = it + (r - 1) * g4 - 1, ir = it + (r - 1) * g4 + 1;
      const u32 l = s_r[il < 0 ? 0 : il], c = s_r[it + (r - 1) * g4], rt = s_r[ir < n4 ? ir : n4 - 1];
      win[r][0] = (int)(l >> 24);
#pragma unroll
      for (int k = 0; k < 4; ++k) win[r][1 + k] = (int)((c >> (8 * k)) & 255u);
      win[r][5] = (int)(rt & 255u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = !((k == 0 && xg == 0) || (k == 3 && xg == g4 - 1));
      const int c = win[1][1 + k];
      const int diff = (int)((od >> (8 * k)) & 255u) - c;
      tot += valid ? diff : 0;
      npx += valid ? 1 : 0;
      const u32 v = (u32)(diff + 255);
      // neighbour pairs of the four classes (g_sao_edge_offsets, sao.h:58-63)
      const int na[4] = { win[1][k], win[0][1 + k], win[0][k], win[0][2 + k] };
      const int nb[4] = { win[1][2 + k], win[2][1 + k], win[2][2 + k], win[2][k] };
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s1 = clampi(c - na[e], -1, 1), s2 = clampi(c - nb[e], -1, 1);
        u32 sel = (u32)(s1 + s2) + 0x0c0c0c02u;                         // byte 0 = index + 2, other selector bytes = constant zero
        if (k == 0 || k == 3) sel = valid ? sel : 0x0c0c0c02u;
        const u32 shs = __builtin_amdgcn_perm(0x0000002Du, 0x1E3C0F00u, sel);    // index -2, -1, 0, 1, 2 -> bit 0, 15, 60, 30, 45
        const u32 shc = __builtin_amdgcn_perm(0x00000015u, 0x0E1C0700u, sel);    //                        -> bit 0, 7, 28, 14, 21
        sum[e] += (unsigned long long)v << shs;
        cnt[e] += 1u << shc;
      }
    }
  }
  // unpack and reduce over the wave: slots -2, -1, +1, +2 are categories 1, 2, 3, 4; category 0 is what is left of the totals
  const int wt = wave_sum(tot), wn = wave_sum(npx);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int rest_s = wt, rest_c = wn;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = (int)((cnt[e] >> (7 * k)) & 127u);
      const int sm = (int)((sum[e] >> (15 * k)) & 32767u) - 255 * c;
      const int ws = wave_sum(sm), wc = wave_sum(c);
      rest_s -= ws; rest_c -= wc;
      if (lane == 0) { atomicAdd(&s_out[e * 10 + 1 + k], ws); atomicAdd(&s_out[e * 10 + 5 + 1 + k], wc); }
    }
    if (lane == 0) { atomicAdd(&s_out[e * 10], rest_s); atomicAdd(&s_out[e * 10 + 5], rest_c); }
  }
  __syncthreads();

  // ---- the record's band half, and the candidates from the finished tables: one lane per band and per (class, category) ----
  if (tid < 32) {
    int c = 0, s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const u32 v = s_hist[w][tid]; c += (int)(v >> 20); s += (int)(v & 0xFFFFFu); }
    s -= 255 * c;
    s_out[40 + tid] = s;
    s_out[72 + tid] = c;
    // calc_sao_band_offsets (sao.c:201-223): the loop from the rounded mean towards zero compares with a best_dist that stays
    // INT_MAX, so every visited offset is stored and the last one visited, +-1, is what remains
    const int o = mean_offset(s, c), last = o > 0 ? 1 : (o < 0 ? -1 : 0);
    s_boff[tid] = last;
    s_dist[tid] = last ? c - 2 * last * s : 0;
  }
  int dd = 0;
  if (tid < 16) {
    // sao_search_edge_sao (sao.c:368-397) for one buffer: sharpening offsets cannot be coded
    const int e = tid >> 2, cat = 1 + (tid & 3);
    const int s = s_out[e * 10 + cat], c = s_out[e * 10 + 5 + cat];
    int o = mean_offset(s, c);
    if (cat <= 2 ? o < 0 : o > 0) o = 0;
    s_cand[e * 5 + cat] = o;
    dd = c * o * o - 2 * o * s;
  }
  if (tid < 64) {
    dd = (int)group_sum<4>((u32)dd);
    if (tid < 16 && (tid & 3) == 0) s_cand[20 + (tid >> 2)] = dd;
    if (tid < 4) s_cand[tid * 5] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    // the first minimum over the 28 windows of four bands (sao.c:226-233)
    int best = 0x7fffffff, pos = 0;
    for (int b = 0; b < 28; ++b) {
      const int d = s_dist[b] + s_dist[b + 1] + s_dist[b + 2] + s_dist[b + 3];
      if (d < best) { best = d; pos = b; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cand[24 + k] = s_boff[pos + k];
    s_cand[28] = pos;
    s_cand[29] = best;
  }
  __syncthreads();
  if (tid < 104) a.stats[(size_t)blockIdx.x * 104 + tid] = s_out[tid];
  if (a.cands && tid < 30) a.cands[(size_t)blockIdx.x * 30 + tid] = s_cand[tid];
}

}  // namespace

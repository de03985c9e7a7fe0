// sao_frame.hip -- sample adaptive offset of a whole picture: per-LCU statistics with the bit-independent candidates, and the
// reconstruction of every LCU and plane.  The stage after kvz_hip_deblock_frame in the picture chain.
//
// Reference: sao_search_luma / sao_search_chroma (sao.c:580-644) for the block geometry, calc_sao_edge_dir (sao-generic.c:82-109),
// calc_sao_bands (sao.c:247-261), sao_search_edge_sao (sao.c:355-400) and calc_sao_band_offsets (sao.c:188-240) without their
// mode bits; kvz_sao_reconstruct (sao.c:278-337) as encoder_sao_reconstruct (encoderstate.c:245-441) applies it.
//
// Statistics: one workgroup per (plane, LCU).  The LCU's rec block is staged in LDS once (dword loads: planes and strides are
// 4-byte aligned, block origins multiples of 32); a work item is one dword of rec with the 3 x 3 dwords around it, so the four
// edge classes and the band histogram all come from that one staging and the source is read once, straight from memory.  The
// edge classes use the packed accumulators of sao.hip's one-wave kernel (fields of a register per category, found with v_perm),
// reduced inside the wave before a handful of LDS atomics across the four waves; the band histogram is one packed LDS counter per
// (wave, band), with runs of equal bands inside a dword merged first.  Everything is integer: no result depends on scheduling.
//
// Reconstruction: one launch for Y, U and V; a workgroup's tile (64 x 16 luma, 32 x 32 chroma pixels, one dword per thread) lies
// inside one LCU, so the SAO record is workgroup-uniform.  Band and copy tiles go from a dword load to a dword store; an edge
// tile is staged in LDS with its one-pixel ring (read across LCU boundaries from the deblocked plane) once.
#include "kvz_hip_internal.h"

using namespace kvzhip;

namespace {

// sao_calc_eo_cat (sao-generic.c:34-43)
__device__ __forceinline__ int eo_cat(int a, int b, int c)
{
  const int idx = 2 + ((c > a) - (c < a)) + ((c > b) - (c < b));
  return (int)((0x43021u >> (4 * idx)) & 15u);          // {1, 2, 0, 3, 4} packed in nibbles
}

__device__ __forceinline__ int wave_sum(int v) { return (int)group_sum<64>((u32)v); }

struct stats_args {
  const u8 *src[3], *rec[3];
  u32 src_stride[2], rec_stride[2];       // [0] luma, [1] chroma
  int width, height, lcus_x, n_lcu;
  int *stats, *cands;                     // 104 / 30 int32 per record; cands may be NULL
};

// offset of one category or band: the mean error rounded to nearest with C's truncating division, clipped to SAO_ABS_OFFSET_MAX
// at bit depth 8 (sao.c:205-206, :381-382)
__device__ __forceinline__ int mean_offset(int sum, int cnt)
{
  return cnt ? clampi((sum + (cnt >> 1)) / cnt, -7, 7) : 0;
}

__global__ __launch_bounds__(256) void sao_stats_frame_kernel(stats_args a)
{
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
  const u32 rs = a.rec_stride[sh], os = a.src_stride[sh];
  const u8 *rec = a.rec[color] + (size_t)y0 * rs + x0;
  const u8 *org = a.src[color] + (size_t)y0 * os + x0;
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

struct frame_args {
  const u8 *rec[3];
  u8 *dst[3];
  u32 rec_stride[2], dst_stride[2];       // [0] luma, [1] chroma
  int width, height, lcus_x, tiles_y, tiles_c;
  const kvz_hip_sao_info *sao[2];         // [0] luma, [1] chroma records
};

// one dword of an edge-offset tile.  s: the tile with its ring, `pitch` dwords per row; at: the dword's index in it.
template <int CLS>
__device__ __forceinline__ u32 edge_dword(const u32 *s, int pitch, int at, int gx, int gy, int pw, int ph, const int *off)
{
  constexpr int RA = CLS == 0 ? 1 : 0;                         // window row of neighbour a; b lies opposite (sao.h:58-63)
  constexpr int DXA = CLS == 1 ? 0 : (CLS == 3 ? 1 : -1);      // its column step
  int win[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (CLS == 0 && r != 1) continue;
    const u32 l = s[at + (r - 1) * pitch - 1], c = s[at + (r - 1) * pitch], rt = s[at + (r - 1) * pitch + 1];
    win[r][0] = (int)(l >> 24);
#pragma unroll
    for (int k = 0; k < 4; ++k) win[r][1 + k] = (int)((c >> (8 * k)) & 255u);
    win[r][5] = (int)(rt & 255u);
  }
  // a pixel whose neighbour a or b lies outside the plane keeps its value: the row / column trimming of sao.c:297-324
  const bool oky = CLS == 0 || (gy >= 1 && gy <= ph - 2);
  u32 out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = gx + k, c = win[1][1 + k];
    const bool ok = oky && (DXA == 0 || (px >= 1 && px <= pw - 2));
    const int cat = eo_cat(win[RA][1 + k + DXA], win[2 - RA][1 + k - DXA], c);
    out |= (u32)(ok ? clampi(c + off[cat], 0, 255) : c) << (8 * k);
  }
  return out;
}

__global__ __launch_bounds__(256) void sao_frame_kernel(frame_args a)
{
  __shared__ u32 s_t[10 * 34];              // the larger of 18 x 18 (luma) and 10 x 34 (chroma) dwords
  const int tid = threadIdx.x;
  int b = (int)blockIdx.x, plane = 0;
  if (b >= a.tiles_y) { b -= a.tiles_y; plane = 1; if (b >= a.tiles_c) { b -= a.tiles_c; plane = 2; } }
  const int sh = plane ? 1 : 0, pw = a.width >> sh, ph = a.height >> sh;
  const int tw = plane ? 8 : 16, th = plane ? 32 : 16;         // tile: dwords x rows
  const int tr = b / a.lcus_x, lx = b - tr * a.lcus_x;
  const int tx0 = lx * 4 * tw, ty0 = tr * th;
  const int lcu = (plane ? tr : (ty0 >> 6)) * a.lcus_x + lx;
  const kvz_hip_sao_info &sao = (plane ? a.sao[1] : a.sao[0])[lcu];
  const int is_v = plane == 2, bp = sao.band_position[is_v], cls = sao.eo_class;
  // the plane's five offsets, looked up per pixel: in LDS (a register array indexed by category would live in scratch)
  __shared__ int s_off[5];
  if (tid < 5) s_off[tid] = sao.offsets[5 * is_v + tid];
  // a malformed record is SAO_TYPE_NONE
  const int mode = (sao.type == 1 && bp >= 0 && bp <= 31) ? 1 : ((sao.type == 2 && cls >= 0 && cls <= 3) ? 2 : 0);

  // selected, not indexed: a dynamically indexed kernel argument array is copied to scratch
  const u32 rs = plane ? a.rec_stride[1] : a.rec_stride[0], ds = plane ? a.dst_stride[1] : a.dst_stride[0];
  const u8 *rec = plane == 0 ? a.rec[0] : (plane == 1 ? a.rec[1] : a.rec[2]);
  u8 *dst = plane == 0 ? a.dst[0] : (plane == 1 ? a.dst[1] : a.dst[2]);
  const int c = tid & (tw - 1), r = tid / tw;
  const int gx = tx0 + 4 * c, gy = ty0 + r;
  const bool inside = gx < pw && gy < ph;
  u32 out = 0;
  if (mode == 2) {
    const int pitch = tw + 2, total = pitch * (th + 2);
    for (int i = tid; i < total; i += 256) {
      const int rr = i / pitch, yy = ty0 + rr - 1, xx = tx0 + 4 * (i - rr * pitch - 1);
      s_t[i] = (yy >= 0 && yy < ph && xx >= 0 && xx < pw) ? *(const u32 *)(rec + (size_t)yy * rs + xx) : 0u;
    }
    __syncthreads();
    if (!inside) return;
    const int at = (r + 1) * pitch + c + 1;
    switch (cls) {
      case 0: out = edge_dword<0>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
      case 1: out = edge_dword<1>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
      case 2: out = edge_dword<2>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
      default: out = edge_dword<3>(s_t, pitch, at, gx, gy, pw, ph, s_off); break;
    }
  } else {
    if (mode == 1) __syncthreads();
    if (!inside) return;
    out = *(const u32 *)(rec + (size_t)gy * rs + gx);
    if (mode == 1) {
      // kvz_calc_sao_offset_array (sao.c:164-180) per pixel
      const u32 in = out;
      out = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int val = (int)((in >> (8 * k)) & 255u), band = (val >> 3) - bp;
        const int o = (band >= 0 && band < 4) ? s_off[(band & 3) + 1] : 0;
        out |= (u32)clampi(val + o, 0, 255) << (8 * k);
      }
    }
  }
  *(u32 *)(dst + (size_t)gy * ds + gx) = out;
}

bool picture_ok(int width, int height)
{
  return width >= 8 && height >= 8 && !((width | height) & 7) && width <= 16384 && height <= 16384;
}

bool plane_ok(const void *p, uint32_t stride, int w)
{
  return p && !((uintptr_t)p & 3) && !(stride & 3) && stride >= (uint32_t)w;
}

}  // namespace

extern "C" {

int kvz_hip_sao_stats_frame(const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                            const kvz_hip_pixel *rec_v, uint32_t stride_c, int chroma, kvz_hip_sao_lcu_stats *stats,
                            kvz_hip_sao_lcu_cand *cands, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!src || !stats || ((uintptr_t)stats & 3) || ((uintptr_t)cands & 3)) return kvzhip::invalid_arg(__func__);
  const int width = src->width, height = src->height;
  if (!picture_ok(width, height) || !plane_ok(src->y, src->stride_y, width) || !plane_ok(rec_y, stride_y, width)) {
    set_error_msg("kvz_hip_sao_stats_frame: planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8");
    return KVZ_HIP_ERR_INVALID;
  }
  if (chroma && (!plane_ok(src->u, src->stride_c, width >> 1) || !plane_ok(src->v, src->stride_c, width >> 1) ||
                 !plane_ok(rec_u, stride_c, width >> 1) || !plane_ok(rec_v, stride_c, width >> 1)))
    return kvzhip::invalid_arg(__func__);
  stats_args a;
  a.src[0] = src->y; a.src[1] = chroma ? src->u : nullptr; a.src[2] = chroma ? src->v : nullptr;
  a.rec[0] = rec_y; a.rec[1] = chroma ? rec_u : nullptr; a.rec[2] = chroma ? rec_v : nullptr;
  a.src_stride[0] = src->stride_y; a.src_stride[1] = src->stride_c;
  a.rec_stride[0] = stride_y; a.rec_stride[1] = stride_c;
  a.width = width; a.height = height;
  a.lcus_x = (width + 63) >> 6;
  a.n_lcu = a.lcus_x * ((height + 63) >> 6);
  a.stats = (int *)stats; a.cands = (int *)cands;
  hipLaunchKernelGGL(sao_stats_frame_kernel, dim3((unsigned)(a.n_lcu * (chroma ? 3 : 1))), dim3(256), 0, ctx_stream(s), a);
  KVZ_CHECK_LAUNCH("sao_stats_frame_kernel");
  return KVZ_HIP_OK;
}

int kvz_hip_sao_frame(const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v, uint32_t stride_c,
                      kvz_hip_pixel *dst_y, uint32_t dst_stride_y, kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v, uint32_t dst_stride_c,
                      int width, int height, const kvz_hip_sao_info *sao_luma, const kvz_hip_sao_info *sao_chroma, int chroma,
                      kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!sao_luma || ((uintptr_t)sao_luma & 3) || dst_y == rec_y) return kvzhip::invalid_arg(__func__);
  if (!picture_ok(width, height) || !plane_ok(rec_y, stride_y, width) || !plane_ok(dst_y, dst_stride_y, width)) {
    set_error_msg("kvz_hip_sao_frame: planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8");
    return KVZ_HIP_ERR_INVALID;
  }
  if (chroma && (!sao_chroma || ((uintptr_t)sao_chroma & 3) || dst_u == rec_u || dst_v == rec_v ||
                 !plane_ok(rec_u, stride_c, width >> 1) || !plane_ok(rec_v, stride_c, width >> 1) ||
                 !plane_ok(dst_u, dst_stride_c, width >> 1) || !plane_ok(dst_v, dst_stride_c, width >> 1)))
    return kvzhip::invalid_arg(__func__);
  frame_args a;
  a.rec[0] = rec_y; a.rec[1] = chroma ? rec_u : nullptr; a.rec[2] = chroma ? rec_v : nullptr;
  a.dst[0] = dst_y; a.dst[1] = chroma ? dst_u : nullptr; a.dst[2] = chroma ? dst_v : nullptr;
  a.rec_stride[0] = stride_y; a.rec_stride[1] = stride_c;
  a.dst_stride[0] = dst_stride_y; a.dst_stride[1] = dst_stride_c;
  a.width = width; a.height = height;
  a.lcus_x = (width + 63) >> 6;
  a.tiles_y = a.lcus_x * ((height + 15) >> 4);
  a.tiles_c = chroma ? a.lcus_x * ((height + 63) >> 6) : 0;
  a.sao[0] = sao_luma; a.sao[1] = chroma ? sao_chroma : nullptr;
  hipLaunchKernelGGL(sao_frame_kernel, dim3((unsigned)(a.tiles_y + 2 * a.tiles_c)), dim3(256), 0, ctx_stream(s), a);
  KVZ_CHECK_LAUNCH("sao_frame_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"

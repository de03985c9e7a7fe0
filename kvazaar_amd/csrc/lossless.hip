// lossless.hip -- kvz_hip_inter_residual_frame_lossless and kvz_hip_intra_recon_frame_lossless: the two residual stages of the picture
// chain for a picture coded with --lossless (quantize_tr_residual's `if (cfg->lossless)` branch, transform.c:354-369, over
// bypass_transquant and rdpcm, transform.c:73-123).
//
// Nothing is transformed or quantised: coeff = source - prediction, rec = source.  In the reference a lossless picture's reconstruction
// IS its source (encoder_set_source_picture, encoderstate.c:1125-1127, and bypass_transquant writes rec = ref for every TU), so every
// reference pixel an intra TU reads equals the source pixel at that place, whatever was coded before it, and availability follows
// position alone.  The intra stage therefore has no dependency between TUs: it takes its reference pixels from the SOURCE plane and
// needs neither the wavefront of launches nor the chain of dependent TUs of intra_recon.hip.  Each entry is ONE launch, Y, U and V
// together, whatever the picture size and the map.
//
// Work unit: a workgroup per LCU (LL_WAVES waves), a wave per 16x16 luma area with the 8x8 areas of U and V below it.
//   * A CU never leaves its LCU, so every CU's cost record, every SCU's cbf_out byte and every TU's flag has one owner: the sums and
//     the flags are gathered in LDS with integer atomics (the result does not depend on their order) and each output is stored once,
//     plainly.  No global atomic, no zeroing pass, no second launch.
//   * A lane owns one row of four pixels of a 4x4 block; the blocks of the area are numbered in z-order, so the lanes of a TU are
//     consecutive: 4 for a 4x4 TU, 16 for 8x8, the whole wave for 16x16 and for a quarter of 32x32.  Sixteen 4x4 TUs (an area of NxN
//     CUs) are predicted side by side, each by its own four lanes: no TU has the wave to itself.  The lanes of a TU build its
//     reference arrays in the wave's LDS slice, then every lane predicts its own four pixels with the functions of intra_core.h.
//   * A TU's flag is a ballot over its lanes; its sums are lane-group reductions (DPP) of integers.
//   * The lane's four pixels are one dword of each plane (any address: lcu_layout.h), its four coefficients one 8-byte store at
//     their place in the TU's contiguous w * w values.
//   * DPCM (implicit_rdpcm, modes 10 and 26) needs the neighbour's residual.  Both modes copy one reference pixel along the DPCM
//     direction (displacement 0) and under implicit_rdpcm the boundary filter is off (intra.c:621), so the neighbour's prediction is
//     the lane's own and its residual is the neighbouring SOURCE pixel minus that: no exchange between lanes, and none between the
//     four waves of a 32x32 TU.
#include "kvz_hip_internal.h"
#include "lcu_layout.h"
#include "intra_core.h"
#include "tile_grid.h"
#include "intra_recon_core.h"

static_assert(sizeof(kvz_hip_lossless) == 16, "layout documented in kvz_hip.h");

namespace {

constexpr int LL_WAVES = 8, LL_WG = 64 * LL_WAVES;

struct ll_args {
  const u8 *src[3];
  u8 *rec[3];
  u32 src_stride[3], rec_stride[3];
  i16 *coeff[3];
  u32 *cus;                      // records as five dwords; cbf_y is byte 4
  const u8 *modes;               // two bytes per SCU (intra entry)
  u8 *cbf_out;                   // or nullptr
  u32 *cost;                     // six dwords per SCU, or nullptr
  int cus_stride, lcus_x;
  int width, height;
  int chroma, rdpcm;
};

// the rule of inter_cu_at (inter_residual_core.h), on the record's first dword
__device__ __forceinline__ bool inter_cu_of(u32 head, int x, int y, int width, int height, int &cu_x, int &cu_y, int &leaf)
{
  const int depth = (head >> 8) & 255, trd = (int)(head >> 24);
  if ((head & 255u) != 2u || depth > 3) return false;                         // CU_INTER (cu.h:38-43)
  const int size = 64 >> depth;
  cu_x = x & ~(size - 1);
  cu_y = y & ~(size - 1);
  leaf = 64 >> min(4, max(max(depth, trd), 1));
  return cu_x + size <= width && cu_y + size <= height;
}

template <bool INTRA>
__device__ __forceinline__ bool own_cu_of(u32 head, int x, int y, int width, int height, int &cu_x, int &cu_y, int &leaf)
{
  if constexpr (INTRA) return intra_cu_of(head, x, y, width, height, cu_x, cu_y, leaf);
  else return inter_cu_of(head, x, y, width, height, cu_x, cu_y, leaf);
}

// Sum over the aligned group of g consecutive lanes that holds the lane, g = 4, 16 or 64 and different from lane to lane: the
// butterfly of group_sum (kvz_hip_internal.h), read off after two, four and six steps.  Every lane of the wave takes part.
__device__ __forceinline__ u32 seg_sum(u32 v, int g)
{
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  const u32 s4 = v;
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  const u32 s16 = v;
  v += (u32)__shfl_xor((int)v, 16, 64);
  v += (u32)__shfl_xor((int)v, 32, 64);
  return g == 4 ? s4 : (g == 16 ? s16 : v);
}

__device__ __forceinline__ int ext_at(const u8 (*ref)[RS], bool fil, const ang_t &an, int idx, int n)
{
  return n == 4 ? ext_entry<4>(ref, fil, an, idx) : n == 8 ? ext_entry<8>(ref, fil, an, idx)
       : n == 16 ? ext_entry<16>(ref, fil, an, idx) : ext_entry<32>(ref, fil, an, idx);
}

// kvz_intra_predict (intra.c:281-331) for pixel (x, y) of a TU n wide, from its staged references: the arithmetic of intra_tu
// (intra_recon_core.h) per pixel, with the extended reference looked up instead of staged
__device__ __forceinline__ int ll_pred_px(const u8 (*ref)[RS], int n, int log2, int mode, int flags, int dc, int x, int y)
{
  const bool fil = use_filtered(mode, log2, flags), edge = luma_edge_filters(log2, flags);
  if (mode >= 2) {
    const ang_t an = ang_of(mode);
    const int r = an.vertical ? y : x, c = an.vertical ? x : y;
    const int pos = (r + 1) * an.disp, di = pos >> 5, f = pos & 31;
    int v = ext_at(ref, fil, an, c + di, n);
    if (f) v = ((32 - f) * v + f * ext_at(ref, fil, an, c + di + 1, n) + 16) >> 5;       // ang_px: f == 0 is e[c + di] itself
    if (edge && (flags & KVZ_HIP_INTRA_FILTER_BOUNDARY) && an.disp == 0 && c == 0) v = post_px(v, ref[2 * fil + (an.vertical ? 0 : 1)], r);
    return v;
  }
  if (mode == 1) return dc_px(ref, dc, edge, x, y);
  return planar_px(ref[2 * fil], ref[2 * fil + 1], n, log2, x, y);
}

// One pass of a wave over its area in one plane.  (lx, ly): the luma position whose record the lane follows -- its 4x4 block in luma,
// the 8x8 area over its 4x4 block in chroma; (px, py): the lane's four pixels in the plane; in: the lane has pixels in this pass.
// Called by the whole wave; the lane-group operations sit outside every divergent branch.
template <bool INTRA>
__device__ __forceinline__ void ll_pass(const ll_args &a, const tile_rect &tr, u8 (*refs)[4][RS], u32 *s_flag, u32 *s_cost, int plane, bool in,
                                        int lx, int ly, int px, int py, int lane)
{
  const int sh = plane ? 1 : 0;
  int cu_x = 0, cu_y = 0, leaf = 4;
  bool on = in && lx < a.width && ly < a.height;
  if (on) on = own_cu_of<INTRA>(a.cus[((size_t)(ly >> 2) * a.cus_stride + (lx >> 2)) * 5], lx, ly, a.width, a.height, cu_x, cu_y, leaf);
  // chroma TUs are half as wide; with 4x4 luma TUs the chroma of the 8x8 area is one 4x4 TU (transform.c:293-313)
  const int n = plane ? (leaf > 8 ? leaf >> 1 : 4) : leaf, log2 = n == 4 ? 2 : n == 8 ? 3 : n == 16 ? 4 : 5;
  const int al = plane ? max(leaf, 8) : leaf;                                  // the TU's alignment in luma pixels
  const int tlx = lx & ~(al - 1), tly = ly & ~(al - 1);
  int mode = 0;
  if constexpr (INTRA) {
    if (on) {
      mode = a.modes[2 * ((size_t)(tly >> 2) * a.cus_stride + (tlx >> 2)) + (plane ? 1 : 0)];
      on = mode <= 34;
    }
  }
  const int tpx = tlx >> sh, tpy = tly >> sh, rx = px - tpx, ry = py - tpy;
  // the TU's lanes in this wave: consecutive, aligned
  const int g = min(n * n / 4, plane ? 16 : 64), g0 = lane & ~(g - 1), li = lane - g0;

  u32 sw[1] = { 0u }, pw[1] = { 0u };
  const size_t s_stride = a.src_stride[plane], r_stride = a.rec_stride[plane];
  const u8 *S = a.src[plane];
  if (on) load_row<4>(S + (size_t)py * s_stride + px, sw);

  if constexpr (INTRA) {
    // ---- kvz_intra_build_reference (intra.c:334-588) from the SOURCE plane, by the rules of intra_tu: the TU's lanes share its 4n + 1 pixels
    u8 (*ref)[RS] = refs[g0 >> 2];
    const int flags = plane == 0 ? (KVZ_HIP_INTRA_LUMA | (a.rdpcm ? 0 : KVZ_HIP_INTRA_FILTER_BOUNDARY)) : 0;      // intra.c:621
    if (on) {
      const int ux = (tlx & 63) >> 2, uy = (tly & 63) >> 2;
      const bool has_left = tlx > tr.x0, has_top = tly > tr.y0;
      const int avail_l = min(intra_coded_left(ux, uy) >> sh, min(2 * n, (tr.y1 - tly) >> sh));
      const int avail_t = min(intra_coded_above(ux, uy) >> sh, min(2 * n, (tr.x1 - tlx) >> sh));
      for (int e = li; e <= 4 * n; e += g) {
        const int i = e < 2 * n ? e : e - 2 * n;
        int v;
        if (e < 2 * n) {
          if (has_left) v = S[(size_t)(tpy + min(i, avail_l - 1)) * s_stride + tpx - 1];
          else v = has_top ? S[(size_t)(tpy - 1) * s_stride + tpx] : 128;
          ref[0][1 + i] = (u8)v;
        } else if (e < 4 * n) {
          if (has_top) v = S[(size_t)(tpy - 1) * s_stride + tpx + min(i, avail_t - 1)];
          else v = has_left ? S[(size_t)tpy * s_stride + tpx - 1] : 128;
          ref[1][1 + i] = (u8)v;
        } else {
          if (has_left && has_top) v = S[(size_t)(tpy - 1) * s_stride + tpx - 1];
          else if (has_left) v = S[(size_t)tpy * s_stride + tpx - 1];
          else v = has_top ? S[(size_t)(tpy - 1) * s_stride + tpx] : 128;
          ref[0][0] = (u8)v;
          ref[1][0] = (u8)v;
        }
      }
    }
    wave_lds_fence();
    // smoothed references (intra.c:164-192): read by luma TUs wider than 4 only (use_filtered)
    if (on && plane == 0 && n > 4) {
      for (int i = li; i < 2 * (2 * n + 1); i += g) {
        const int s = i >= 2 * n + 1, e = i - (2 * n + 1) * s;
        const u8 *from = ref[s];
        int v;
        if (e == 0) v = (ref[0][1] + 2 * ref[0][0] + ref[1][1] + 2) >> 2;
        else if (e == 2 * n) v = from[e];
        else v = (from[e - 1] + 2 * from[e] + from[e + 1] + 2) >> 2;
        ref[2 + s][e] = (u8)v;
      }
    }
    wave_lds_fence();
    if (on) {
      const int dc = mode == 1 ? dc_value(ref, n, log2) : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) pw[0] |= (u32)ll_pred_px(ref, n, log2, mode, flags, dc, rx + i, ry) << (8 * i);
    }
    wave_lds_fence();                                                            // the slice is free for the next pass
  } else {
    if (on) load_row<4>(a.rec[plane] + (size_t)py * r_stride + px, pw);         // the prediction, in place
  }

  // ---- bypass_transquant (transform.c:73-100) and rdpcm (transform.c:109-123)
  u32 zssd = 0, sab = 0;
  int any = 0;
  if (on) {
    int c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = byte_of(sw, i) - byte_of(pw, i);
      zssd += (u32)(c[i] * c[i]);
    }
    if constexpr (INTRA) {
      // transform.c:362-368.  The reference walks from the bottom right, so every subtraction sees the unmodified neighbour; here the
      // neighbour's residual is made from the source (see the head of the file)
      if (a.rdpcm && mode == 10) {
        const int left = rx > 0 ? (int)S[(size_t)py * s_stride + px - 1] - byte_of(pw, 0) : 0;
        const int r0 = c[0], r1 = c[1], r2 = c[2];
        c[0] -= left; c[1] -= r0; c[2] -= r1; c[3] -= r2;
      } else if (a.rdpcm && mode == 26 && ry > 0) {
        u32 up[1];
        load_row<4>(S + (size_t)(py - 1) * s_stride + px, up);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] -= byte_of(up, i) - byte_of(pw, i);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sab += (u32)(c[i] < 0 ? -c[i] : c[i]);
      any |= c[i];
    }
    const int bx = (tlx & 63) >> (2 + sh), by = (tly & 63) >> (2 + sh);
    const size_t lcu = (size_t)(ly >> 6) * a.lcus_x + (lx >> 6);
    i16 *dst = a.coeff[plane] + lcu * (plane ? 1024 : 4096) + 16 * zorder_blk(bx, by) + ry * n + rx;
    *(uint2 *)dst = make_uint2(((u32)c[0] & 0xffffu) | ((u32)c[1] << 16), ((u32)c[2] & 0xffffu) | ((u32)c[3] << 16));
    store_row<4>(a.rec[plane] + (size_t)py * r_stride + px, sw);                 // rec = source
  }
  // has_coeffs (taken before the DPCM in the reference; DPCM is invertible, so "any stored value non-zero" is the same): a vote of the
  // TU's lanes.  The waves of a 32x32 TU meet in s_flag, like the planes of an SCU
  const unsigned long long votes = __ballot(on && any != 0);
  const unsigned long long mine = g == 64 ? ~0ull : (((1ull << g) - 1ull) << g0);
  const bool has = (votes & mine) != 0ull;
  zssd = seg_sum(on ? zssd : 0u, g);
  sab = seg_sum(on ? sab : 0u, g);
  if (on && li == 0) {
    // bit `plane`: has_coeffs; bit 4 + plane: the TU was coded.  At the SCU of the TU's luma origin inside the LCU
    atomicOr(&s_flag[((tly & 63) >> 2) * 16 + ((tlx & 63) >> 2)], ((has ? 1u : 0u) | 16u) << plane);
    u32 *cst = s_cost + (((cu_y & 63) >> 2) * 16 + ((cu_x & 63) >> 2)) * 6 + sh;
    atomicAdd(cst + 2, zssd);                                                    // ssd_* stays 0: the reconstruction is the source
    atomicAdd(cst + 4, sab);
  }
}

// grid: one workgroup per LCU, raster order
template <bool INTRA>
__global__ __launch_bounds__(LL_WG) void lossless_lcu_kernel(ll_args a, kvz_hip_tile_grid grid)
{
  __shared__ __attribute__((aligned(16))) u8 s_ref[INTRA ? LL_WAVES : 1][16][4][RS];   // per wave: a slot per 4x4 block; a TU uses its first block's
  __shared__ u32 s_flag[256];
  __shared__ u32 s_cost[256 * 6];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcu_y = (int)blockIdx.x / a.lcus_x, lcu_x = (int)blockIdx.x - lcu_y * a.lcus_x;
  const int X0 = 64 * lcu_x, Y0 = 64 * lcu_y;
  for (int i = tid; i < 256; i += LL_WG) s_flag[i] = 0u;
  for (int i = tid; i < 256 * 6; i += LL_WG) s_cost[i] = 0u;
  __syncthreads();

  // the rectangle that stands for the picture in everything about an intra TU's neighbours: the LCU's tile (wave-uniform)
  tile_rect tr = { 0, 0, a.width, a.height };
  if constexpr (INTRA) {
    int cx0, cx1, ry0, ry1;
    tile_span_of(grid.col_bd, grid.cols, lcu_x, cx0, cx1);
    tile_span_of(grid.row_bd, grid.rows, lcu_y, ry0, ry1);
    tr = { 64 * cx0, 64 * ry0, min(64 * cx1, a.width), min(64 * ry1, a.height) };
  }

  for (int area = wave; area < 16; area += LL_WAVES) {
    const int AX = X0 + 16 * (area & 3), AY = Y0 + 16 * (area >> 2);
    if (AX >= a.width || AY >= a.height) continue;                              // wave-uniform; no workgroup barrier in this loop
    u8 (*refs)[4][RS] = s_ref[INTRA ? wave : 0];
    {
      // luma: lane = 4 * (z-order index of the 4x4 block) + row
      const int b = lane >> 2, x = AX + 4 * compact4(b), y = AY + 4 * compact4(b >> 1);
      ll_pass<INTRA>(a, tr, refs, s_flag, s_cost, 0, true, x, y, x, y + (lane & 3), lane);
    }
    if (a.chroma) {
      // chroma: lanes 0-15 U, 16-31 V; the 4x4 block (bx, by) of the 8x8 area lies under the 8x8 luma area (8 bx, 8 by)
      const int plane = 1 + ((lane >> 4) & 1), b = (lane >> 2) & 3, x = AX + 8 * (b & 1), y = AY + 8 * (b >> 1);
      ll_pass<INTRA>(a, tr, refs, s_flag, s_cost, plane, lane < 32, x, y, x >> 1, (y >> 1) + (lane & 3), lane);
    }
  }
  __syncthreads();

  // ---- every SCU of the LCU once: its flags, and its CU's sums where it is the CU's first
  if (tid < 256) {
    const int x = X0 + 4 * (tid & 15), y = Y0 + 4 * (tid >> 4);
    int cu_x, cu_y, leaf;
    if (x < a.width && y < a.height) {
      const size_t scu = (size_t)(y >> 2) * a.cus_stride + (x >> 2);
      if (own_cu_of<INTRA>(a.cus[scu * 5], x, y, a.width, a.height, cu_x, cu_y, leaf)) {
        const int lc = max(leaf, 8);
        const u32 fl = s_flag[(((y & ~(leaf - 1)) & 63) >> 2) * 16 + (((x & ~(leaf - 1)) & 63) >> 2)];
        const u32 fc = s_flag[(((y & ~(lc - 1)) & 63) >> 2) * 16 + (((x & ~(lc - 1)) & 63) >> 2)];
        if (fl & 16u) ((u8 *)a.cus)[scu * 20 + 4] = (u8)(fl & 1u);                // cbf_y as lcu_set_coeff leaves it (search.c:173-190)
        if (a.cbf_out) a.cbf_out[scu] = (u8)((fl & 1u) | (fc & 6u));
        if (a.cost && cu_x == x && cu_y == y) {
#pragma unroll
          for (int j = 0; j < 6; ++j) a.cost[scu * 6 + j] = s_cost[tid * 6 + j];
        }
      }
    }
  }
}

// p: the entry's arguments as a record (chain_picture_pack), whose params hold ll->chroma and nothing else
int lossless_frame(const char *entry, bool intra, const kvz_hip_chain_picture &p, const kvz_hip_tile_grid *tiles, const kvz_hip_lossless *ll,
                   kvz_hip_stream s)
{
  if (ll->reserved[0] || ll->reserved[1] || !chain_picture_args_ok(p, intra, false)) return kvzhip::invalid_arg(entry);
  const int width = p.src.width, height = p.src.height, chroma = ll->chroma ? 1 : 0;
  kvz_hip_tile_grid grid;
  if (!tile_grid_make(intra ? tiles : nullptr, width, height, &grid)) return kvzhip::invalid_arg(entry);
  ll_args a;
  a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.src_stride[0] = p.src.stride_y; a.src_stride[1] = a.src_stride[2] = p.src.stride_c;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = a.rec_stride[2] = p.stride_c;
  a.coeff[0] = p.coeff_y; a.coeff[1] = chroma ? p.coeff_u : nullptr; a.coeff[2] = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.modes = p.intra_modes; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs;
  a.cus_stride = width >> 2; a.lcus_x = (width + 63) >> 6;
  a.width = width; a.height = height;
  a.chroma = chroma; a.rdpcm = ll->implicit_rdpcm ? 1 : 0;
  const unsigned lcus = (unsigned)(a.lcus_x * ((height + 63) >> 6));
  hipStream_t st = ctx_stream(s);
  // the one launch of the entry: its shape depends on width and height alone
  if (intra) hipLaunchKernelGGL(lossless_lcu_kernel<true>, dim3(lcus), dim3(LL_WG), 0, st, a, grid);
  else hipLaunchKernelGGL(lossless_lcu_kernel<false>, dim3(lcus), dim3(LL_WG), 0, st, a, grid);
  KVZ_CHECK_LAUNCH("lossless_lcu_kernel");
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frame_lossless(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                          kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                          kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                          kvz_hip_inter_residual_cost *costs, const kvz_hip_lossless *ll, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!ll) return kvzhip::invalid_arg(__func__);
  const kvz_hip_inter_residual_params flat = { 0, 0, 0, 0, ll->chroma, 0 };     // what the check of the arguments reads of them
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         nullptr, &flat);
  return packed ? lossless_frame(__func__, false, p, nullptr, ll, s) : kvzhip::invalid_arg(__func__);
}

int kvz_hip_intra_recon_frame_lossless(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                       kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                       kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                       kvz_hip_inter_residual_cost *costs, const kvz_hip_tile_grid *tiles, const kvz_hip_lossless *ll,
                                       kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!ll) return kvzhip::invalid_arg(__func__);
  const kvz_hip_inter_residual_params flat = { 0, 0, 0, 0, ll->chroma, 0 };     // what the check of the arguments reads of them
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, intra_modes, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         nullptr, &flat);
  return packed ? lossless_frame(__func__, true, p, tiles, ll, s) : kvzhip::invalid_arg(__func__);
}

}  // extern "C"

// inter_recon_core.h -- what the motion-compensation kernels share: inter_recon.hip (PU descriptors and one picture) and
// inter_recon_multi.hip (several pictures over a shared pool of reference pictures).
//
// The unit of work is a RECTANGLE of at most 16x16 luma samples with its 8x8 U and V samples, owned by one wave with a
// private LDS slice and no barrier (see inter_recon.hip).  The code is templated on a small VIEW of the picture being
// predicted, so that each kernel hands over what its own arguments hold:
//   refs[]                 the reference pictures a motion's ref[] indexes (kvz_hip_ref_picture; an array or a pointer)
//   n_refs                 how many of them there are: a motion whose used ref[] is not below it is skipped
//   y, u, v                destination planes
//   stride_y, stride_c     their strides
//   width, height          luma size of the picture (= of every reference picture it names)
//   chroma                 0 = 4:0:0
// recon_args (inter_recon.hip) is such a view with the table inside it; recon_view (inter_recon_multi.hip) points at the pool.
// The host side -- ref_ok, the rule for one reference picture of a table, and the checks of a record -- is in chain_host.h.
#pragma once

#include "kvz_hip_internal.h"
#include "frac_core.h"
#include "chain_host.h"

using namespace kvzhip;

namespace {

static_assert(sizeof(kvz_hip_ref_picture) == 40 && sizeof(kvz_hip_inter_pu) == 28 && sizeof(kvz_hip_inter_recon_params) == 40 &&
              sizeof(kvz_hip_cu_info) == 20, "layouts documented in kvz_hip.h");

__constant__ signed char c_chroma_taps[8][4] = {        // filter.c:62-72
  { 0, 64, 0, 0 }, { -2, 58, 10, -2 }, { -4, 54, 16, -2 }, { -6, 46, 28, -4 },
  { -4, 36, 36, -4 }, { -4, 28, 46, -6 }, { -2, 16, 54, -4 }, { -2, 10, 58, -2 } };
// q / d for d = 1..6 and q < 192 as (q * ceil(65536 / d)) >> 16
__constant__ int c_recip[7] = { 0, 65536, 32768, 21846, 16384, 13108, 10923 };
__device__ __forceinline__ int div_small(int q, int d) { return (q * c_recip[d]) >> 16; }

// One wave's LDS slice.  Luma: window rows of 24 bytes (16 + 7 samples, dword rounded), 23 rows; transposed
// horizontal plane, 13 dwords (23 rows, odd: columns start in different banks) for each of 16 columns.  Chroma, per
// plane: window rows of 12 bytes (8 + 3), 11 rows; 7 dwords for each of 8 columns.
constexpr int L_WS = 24, L_HP = 13, C_WS = 12, C_HP = 7;
constexpr int OFF_LWIN = 0, OFF_LHOR = OFF_LWIN + L_WS * 24, OFF_CWIN = OFF_LHOR + 16 * L_HP * 4;
constexpr int C_WIN_BYTES = C_WS * 12, C_HOR_BYTES = 8 * C_HP * 4;
constexpr int OFF_CHOR = OFF_CWIN + 2 * C_WIN_BYTES, LDS_WAVE = OFF_CHOR + 2 * C_HOR_BYTES;
static_assert(LDS_WAVE % 16 == 0 && OFF_LHOR % 16 == 0 && OFF_CWIN % 16 == 0 && OFF_CHOR % 16 == 0, "aligned slices");

struct motion_t { int dir; int ref[2]; int mv[2][2]; };    // the same in every lane of the wave

// Coefficient pairs of the vertical filter for v_dot2: row pair t of the transposed column against taps (2t, 2t + 1)
// for an even output row, (2t - 1, 2t) for an odd one, which starts half a pair later.
template <int TAPS>
__device__ __forceinline__ u32 vcoef(const signed char *vf, int t, int odd)
{
  constexpr int HALF = TAPS / 2;
  const u32 ce = t < HALF ? frac_pack16(vf[2 * t], vf[2 * t + 1]) : 0u;
  const u32 co = frac_pack16(t > 0 ? vf[2 * t - 1] : 0, t < HALF ? vf[2 * t] : 0);
  return odd ? co : ce;
}

// 14-bit luma samples of the lane's 1 x 4 item (row, columns 4 g ..) of the rw x rh rectangle whose integer
// position in `ref` is (ix, iy).  Every lane of the wave takes part in the window load and the horizontal pass.
__device__ __forceinline__ void luma_src14(int lane, u8 *lds, const refplane_t &ref, int ix, int iy, int fx, int fy,
                                           int rw, int rh, int row, int g, bool act, int v[4])
{
  if (!(fx | fy)) {                                     // integer vector: pixels << 6, each coordinate clamped
    if (!act) return;
    if (ix >= 0 && iy >= 0 && ix + rw <= ref.w && iy + rh <= ref.h) {
      u32 d;
      __builtin_memcpy(&d, ref.p + (size_t)(iy + row) * ref.stride + ix + 4 * g, 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (int)((d >> (8 * k)) & 255u) << 6;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (int)ref_px(ref, ix + 4 * g + k, iy + row) << 6;
    }
    return;
  }
  u8 *s_win = lds + OFF_LWIN;
  u32 *s_hor = (u32 *)(lds + OFF_LHOR);
  const int w4 = rw >> 2, ww = rw + 7, wh = rh + 7, x0 = ix - 3, y0 = iy - 3, wq = (ww + 3) >> 2;
  // window rows as (unaligned) dwords when the dword-rounded window lies inside the plane, else byte by byte with
  // edge replication (kvz_get_extended_block, ipol-generic.c:731-784)
  if (x0 >= 0 && y0 >= 0 && x0 + 4 * wq <= ref.w && y0 + wh <= ref.h) {
    for (int i = lane; i < wq * wh; i += 64) {
      const int y = div_small(i, wq), q = i - y * wq;
      u32 d;
      __builtin_memcpy(&d, ref.p + (size_t)(y0 + y) * ref.stride + x0 + 4 * q, 4);
      *(u32 *)(s_win + y * L_WS + 4 * q) = d;
    }
  } else {
    const int x = lane & 31;
    if (x < ww)
      for (int y = lane >> 5; y < wh; y += 2) s_win[y * L_WS + x] = ref_px(ref, x0 + x, y0 + y);
  }
  wave_lds_fence();
  {
    const u32 *fl = (const u32 *)&c_luma_filter[0][0];
    const u32 h0 = fl[2 * fx], h1 = fl[2 * fx + 1];
    for (int i = lane; i < w4 * wh; i += 64) {            // item = window row r x 4 columns
      const int r = div_small(i, w4), gg = i - r * w4;
      const u32 *q = (const u32 *)(s_win + r * L_WS + 4 * gg);
      const u32 d0 = q[0] ^ 0x80808080u, d1 = q[1] ^ 0x80808080u, d2 = q[2] ^ 0x80808080u;
      unsigned short *col = (unsigned short *)(s_hor + 4 * gg * L_HP) + r;     // column x at dword x * L_HP, row r in halfword r
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const u32 lo = k ? __builtin_amdgcn_alignbyte(d1, d0, (u32)k) : d0, hi = k ? __builtin_amdgcn_alignbyte(d2, d1, (u32)k) : d1;
        const int s = __builtin_amdgcn_sdot4((int)h0, (int)lo, __builtin_amdgcn_sdot4((int)h1, (int)hi, 8192, false), false);
        col[k * 2 * L_HP] = (unsigned short)s;
      }
    }
  }
  wave_lds_fence();
  if (act) {
    const signed char *vf = c_luma_filter[fy];
    const int odd = row & 1;
    u32 cf[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) cf[t] = vcoef<8>(vf, t, odd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32 *col = s_hor + (4 * g + k) * L_HP + (row >> 1);
      int acc = 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) acc = __builtin_amdgcn_sdot2(as_v2s(col[t]), as_v2s(cf[t]), acc, false);
      v[k] = (int)(i16)(acc >> 6);
    }
  }
  wave_lds_fence();                                       // the next reference reuses the slice
}

// The same for chroma: lanes 0..31 work on U, 32..63 on V; the lane's item is 1 x 2 samples (row, columns 2 g, 2 g + 1)
// of the cw x ch rectangle (cw 2..8, even) at the integer position (ix, iy) of the chroma planes.
__device__ __forceinline__ void chroma_src14(int lane, u8 *lds, const kvz_hip_ref_picture &rp, int ix, int iy, int fx, int fy,
                                             int cw, int ch, int row, int g, bool act, int v[2])
{
  const int p = lane >> 5, q32 = lane & 31;
  const refplane_t ref = { p ? rp.v : rp.u, rp.stride_c, rp.width >> 1, rp.height >> 1 };
  if (!(fx | fy)) {
    if (!act) return;
    if (ix >= 0 && iy >= 0 && ix + cw <= ref.w && iy + ch <= ref.h) {
      unsigned short d;
      __builtin_memcpy(&d, ref.p + (size_t)(iy + row) * ref.stride + ix + 2 * g, 2);
      v[0] = (int)(d & 255u) << 6;
      v[1] = (int)(d >> 8) << 6;
    } else {
      v[0] = (int)ref_px(ref, ix + 2 * g, iy + row) << 6;
      v[1] = (int)ref_px(ref, ix + 2 * g + 1, iy + row) << 6;
    }
    return;
  }
  u8 *s_win = lds + OFF_CWIN + p * C_WIN_BYTES;
  u32 *s_hor = (u32 *)(lds + OFF_CHOR + p * C_HOR_BYTES);
  const int ww = cw + 3, wh = ch + 3, x0 = ix - 1, y0 = iy - 1, wq = (ww + 3) >> 2;
  if (x0 >= 0 && y0 >= 0 && x0 + 4 * wq <= ref.w && y0 + wh <= ref.h) {
    for (int i = q32; i < wq * wh; i += 32) {
      const int y = div_small(i, wq), q = i - y * wq;
      u32 d;
      __builtin_memcpy(&d, ref.p + (size_t)(y0 + y) * ref.stride + x0 + 4 * q, 4);
      *(u32 *)(s_win + y * C_WS + 4 * q) = d;
    }
  } else {
    const int x = q32 & 15;
    if (x < ww)
      for (int y = q32 >> 4; y < wh; y += 2) s_win[y * C_WS + x] = ref_px(ref, x0 + x, y0 + y);
  }
  wave_lds_fence();
  {
    // columns in groups of 4 (a 2- or 6-wide rectangle fills a group it does not use: reads stay inside the row)
    const int ng = (cw + 3) >> 2;
    const u32 h0 = *(const u32 *)c_chroma_taps[fx];
    if (q32 < ng * wh) {
      const int r = div_small(q32, ng), gg = q32 - r * ng;
      const u32 *q = (const u32 *)(s_win + r * C_WS + 4 * gg);
      const u32 d0 = q[0] ^ 0x80808080u, d1 = q[1] ^ 0x80808080u;
      unsigned short *col = (unsigned short *)(s_hor + 4 * gg * C_HP) + r;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const u32 lo = k ? __builtin_amdgcn_alignbyte(d1, d0, (u32)k) : d0;
        col[k * 2 * C_HP] = (unsigned short)__builtin_amdgcn_sdot4((int)h0, (int)lo, 8192, false);
      }
    }
  }
  wave_lds_fence();
  if (act) {
    const signed char *vf = c_chroma_taps[fy];
    const int odd = row & 1;
    u32 cf[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) cf[t] = vcoef<4>(vf, t, odd);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const u32 *col = s_hor + (2 * g + k) * C_HP + (row >> 1);
      int acc = 0;
#pragma unroll
      for (int t = 0; t < 3; ++t) acc = __builtin_amdgcn_sdot2(as_v2s(col[t]), as_v2s(cf[t]), acc, false);
      v[k] = (int)(i16)(acc >> 6);
    }
  }
  wave_lds_fence();
}

// Prediction of the luma rectangle (rx, ry, rw, rh) -- multiples of 4, at most 16x16, inside the picture -- and of
// its chroma, from the motion m of the PU it belongs to.  rx, ry, rw, rh and m are wave-uniform.
template <class A>
__device__ __forceinline__ void predict_rect(int lane, u8 *lds, const A &a, const motion_t &m, int rx, int ry, int rw, int rh)
{
  const bool bi = m.dir == 3;
  {
    const int w4 = rw >> 2, row = div_small(lane, w4), g = lane - row * w4;
    const bool act = lane < w4 * rh;
    int acc[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!(m.dir & (1 << k))) continue;
      const kvz_hip_ref_picture &rp = a.refs[m.ref[k]];
      const refplane_t ref = { rp.y, rp.stride_y, rp.width, rp.height };
      int v[4] = { 0, 0, 0, 0 };
      luma_src14(lane, lds, ref, rx + (m.mv[k][0] >> 2), ry + (m.mv[k][1] >> 2), m.mv[k][0] & 3, m.mv[k][1] & 3, rw, rh, row, g, act, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += v[j];
    }
    if (act) {
      u32 o = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) o |= (u32)fast_clip32(bi ? (acc[j] + 64) >> 7 : (acc[j] + 32) >> 6) << (8 * j);
      __builtin_memcpy(a.y + (size_t)(ry + row) * a.stride_y + rx + 4 * g, &o, 4);
    }
  }
  if (!a.chroma) return;
  {
    const int cx = rx >> 1, cy = ry >> 1, cw = rw >> 1, ch = rh >> 1, c2 = cw >> 1;
    const int q32 = lane & 31, row = div_small(q32, c2), g = q32 - row * c2;
    const bool act = q32 < c2 * ch;
    int acc[2] = { 0, 0 };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!(m.dir & (1 << k))) continue;
      int v[2] = { 0, 0 };
      // (x >> 1, y >> 1) + ((mv >> 2) >> 1), fraction mv & 7 (inter.c:124-170)
      chroma_src14(lane, lds, a.refs[m.ref[k]], cx + (m.mv[k][0] >> 3), cy + (m.mv[k][1] >> 3), m.mv[k][0] & 7, m.mv[k][1] & 7, cw, ch, row, g, act, v);
      acc[0] += v[0];
      acc[1] += v[1];
    }
    if (act) {
      const unsigned short o = (unsigned short)((u32)fast_clip32(bi ? (acc[0] + 64) >> 7 : (acc[0] + 32) >> 6) |
                                                ((u32)fast_clip32(bi ? (acc[1] + 64) >> 7 : (acc[1] + 32) >> 6) << 8));
      u8 *plane = (lane >> 5) ? a.v : a.u;
      __builtin_memcpy(plane + (size_t)(cy + row) * a.stride_c + cx + 2 * g, &o, 2);
    }
  }
}

// shape, position and motion of a PU that the entries accept; anything else is skipped
template <class A>
__device__ __forceinline__ bool pu_ok(const A &a, int x, int y, int w, int h, const motion_t &m)
{
  if (!frac_shape_ok(w, h) || x < 0 || y < 0 || ((x | y) & 3) || x + w > a.width || y + h > a.height) return false;
  if (m.dir < 1 || m.dir > 3) return false;
  if ((m.dir & 1) && (unsigned)m.ref[0] >= (unsigned)a.n_refs) return false;
  if ((m.dir & 2) && (unsigned)m.ref[1] >= (unsigned)a.n_refs) return false;
  return true;
}

// Split positions of the eight part modes in quarters of the CU width (cu.c:51-78): 2Nx2N, 2NxN, Nx2N, NxN,
// 2NxnU, 2NxnD, nLx2N, nRx2N; 0 = not split along that axis.
__constant__ unsigned char c_split_x[8] = { 0, 0, 2, 2, 0, 0, 1, 3 };
__constant__ unsigned char c_split_y[8] = { 0, 2, 0, 2, 1, 3, 0, 0 };

// A wave takes one 16x16 tile (tx0, ty0) of the picture.  Lane l < 16 looks at the SCU (l & 3, l >> 2) of the tile: its
// record gives the CU (depth), the CU's first record the part mode, and the PU that holds the SCU its motion from the
// record at the PU's own top-left SCU (inter.c:498-507); ref_of[list][mv_ref[list]] is the index into a.refs.  The wave
// then works through the distinct PUs of the tile: the first pending lane's PU, cut to the tile, is predicted and every
// SCU inside that rectangle is retired.  This is the body of inter_recon_frame_kernel (inter_recon.hip), which keeps its
// own copy so that it compiles to the instructions it always had; a change to either belongs in both.
template <class A>
__device__ __forceinline__ void predict_tile(int lane, u8 *lds, const A &a, const u32 *__restrict__ cus, int cus_stride,
                                             const uint8_t (&ref_of)[2][16], int tx0, int ty0)
{
  const int px = tx0 + 4 * (lane & 3), py = ty0 + 4 * ((lane >> 2) & 3);       // the lane's SCU, in pixels
  bool valid = lane < 16 && px < a.width && py < a.height;
  int pu_x = 0, pu_y = 0, pu_w = 0, pu_h = 0, dir = 0, r0 = 255, r1 = 255;
  u32 mv0 = 0, mv1 = 0;
  if (valid) {
    const u32 head = cus[((size_t)(py >> 2) * cus_stride + (px >> 2)) * 5];
    const int depth = (head >> 8) & 255;
    valid = (head & 255u) == 2u && depth <= 3;                             // CU_INTER (cu.h:38-43)
    if (valid) {
      const int size = 64 >> depth, cu_x = px & ~(size - 1), cu_y = py & ~(size - 1);
      valid = cu_x + size <= a.width && cu_y + size <= a.height;
      if (valid) {
        const int part = (cus[((size_t)(cu_y >> 2) * cus_stride + (cu_x >> 2)) * 5] >> 16) & 255;
        valid = part < 8;
        if (valid) {
          const int bx = c_split_x[part] * (size >> 2), by = c_split_y[part] * (size >> 2);
          const int ox = px - cu_x, oy = py - cu_y;
          pu_x = cu_x + (bx && ox >= bx ? bx : 0);
          pu_y = cu_y + (by && oy >= by ? by : 0);
          pu_w = bx ? (ox >= bx ? size - bx : bx) : size;
          pu_h = by ? (oy >= by ? size - by : by) : size;
          valid = ((pu_x | pu_y) & 3) == 0;                                // an 8x8 CU in an AMP mode: no such PU
          if (valid) {
            const u32 *rec = cus + ((size_t)(pu_y >> 2) * cus_stride + (pu_x >> 2)) * 5;
            dir = (rec[1] >> 8) & 255;
            mv0 = rec[2];
            mv1 = rec[3];
            const u32 idx = rec[4];
            const int i0 = idx & 255, i1 = (idx >> 8) & 255;
            r0 = i0 < 16 ? ref_of[0][i0] : 255;
            r1 = i1 < 16 ? ref_of[1][i1] : 255;
            const motion_t m = { dir, { r0, r1 }, { { 0, 0 }, { 0, 0 } } };
            valid = pu_ok(a, pu_x, pu_y, pu_w, pu_h, m);
          }
        }
      }
    }
  }
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int l0 = __builtin_ctzll(todo);
    const int ux = __builtin_amdgcn_readlane(pu_x, l0), uy = __builtin_amdgcn_readlane(pu_y, l0);
    const int uw = __builtin_amdgcn_readlane(pu_w, l0), uh = __builtin_amdgcn_readlane(pu_h, l0);
    const u32 v0 = (u32)__builtin_amdgcn_readlane((int)mv0, l0), v1 = (u32)__builtin_amdgcn_readlane((int)mv1, l0);
    const motion_t m = { __builtin_amdgcn_readlane(dir, l0), { __builtin_amdgcn_readlane(r0, l0), __builtin_amdgcn_readlane(r1, l0) },
                         { { (int)(i16)(v0 & 0xffffu), (int)(i16)(v0 >> 16) }, { (int)(i16)(v1 & 0xffffu), (int)(i16)(v1 >> 16) } } };
    // the PU cut to the tile (the PU lies inside the picture, so the rectangle does too)
    const int rx = max(ux, tx0), ry = max(uy, ty0), rxe = min(ux + uw, tx0 + 16), rye = min(uy + uh, ty0 + 16);
    predict_rect(lane, lds, a, m, rx, ry, rxe - rx, rye - ry);
    todo &= ~__ballot(lane < 16 && px >= rx && px < rxe && py >= ry && py < rye);
  }
}

}  // namespace

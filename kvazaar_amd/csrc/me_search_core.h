// me_search_core.h -- one motion search per PU, entirely on the device: hexagon search with MV bit
// costs, then the fused fractional search.
//
// Reference: the --me hexbs (and --me dia, diamond_search :796-883; --me tz, tz_search :595-672) path of search_pu_inter_ref (src/search_inter.c:1134-1300):
// hexagon_search (:690-778) = select_starting_point (:282-307) + early_terminate (:415-460) +
// the 6/3/8-point patterns, every candidate through check_mv_cost (:195-232) = kvz_image_calc_sad
// (image.c:455-486) + calc_mvd_cost (:373-412); then search_frac (:965-1128).  SURVEY.md 8(f) row 1.
//
// The reference walks each pattern one candidate at a time and keeps the running best with a
// strict '<', i.e. it takes the first minimum of the group in visiting order.  Here the SADs of a
// whole group (up to 8 candidates) are computed at once -- work item = (candidate, 8-pixel row
// segment), spread over the wave / workgroup that owns the PU, partial sums through LDS atomics --
// and the same first-minimum rule is applied to the group, so every decision (and therefore the
// path the search takes) is the reference's.  The current block lives in LDS for the whole search;
// reference pixels come from L2/HBM with the clamp addressing of image_interpolated_sad
// (image.c:320-444).  The fractional stage is frac_core.h with the MV cost model plugged in.
#pragma once
#include "frac_core.h"
#include "me_cost.h"
#include "serve_ring.h"
#include <type_traits>

namespace kvzhip {

static __constant__ signed char c_large_hex[9][2] = { { 0, 0 }, { 1, -2 }, { 2, 0 }, { 1, 2 }, { -1, 2 }, { -2, 0 }, { -1, -2 }, { 1, -2 }, { 2, 0 } };
static __constant__ signed char c_small_hex[9][2] = { { 0, 0 }, { 0, -1 }, { -1, 0 }, { 1, 0 }, { 0, 1 }, { -1, -1 }, { 1, -1 }, { -1, 1 }, { 1, 1 } };
static __constant__ signed char c_diamond[5][2] = { { 0, -1 }, { 1, 0 }, { 0, 1 }, { -1, 0 }, { 0, 0 } };
static __constant__ signed char c_et_hex[7][2] = { { 0, -1 }, { -1, 0 }, { 0, 1 }, { 1, 0 }, { 0, -1 }, { -1, 0 }, { 0, 0 } };

constexpr int ME_GROUP = 64;                          // candidates evaluated per round (the patterns use at most 8)
struct me_shared { u32 sad[ME_GROUP]; int cx[ME_GROUP], cy[ME_GROUP]; };

constexpr int FULL_OUT = 32;                          // me_shared slot where full_search_wg leaves (x, y, cost, bits)
constexpr int FULL_MAX_WINDOWS = 7;                   // zero vector, extra_mv, five merge candidates

// search_mv_full (search_inter.c:886-962) for the search service: ALL threads of the workgroup on the positions of one PU
// and one reference picture, whatever the PU's size -- the latency form of the exhaustive search (the one-wave-per-PU form
// in search_pu_core is the throughput form: 64 positions per round).
//   * the (w + 2R) x (h + 2R) reference pixels of as many windows as fit are staged in LDS at once (edge replicated,
//     image.c:320-444), the current block beside them;
//   * a work item is FOUR neighbouring positions of one window row: v_qsad_pk_u16_u8 prices the four alignments of a
//     reference dword pair against one dword of the block in one instruction (16-bit packed sums, emptied into 32-bit
//     ones before 64 of them can overflow: 64 x 4 x 255 < 2^16); QSAD = false keeps v_alignbyte + v_sad_u8;
//   * the reference walks the windows in order and replaces its best on a strictly smaller cost, so the winner is the
//     smallest (cost, visiting order) pair: every thread keeps its own 64-bit minimum and one reduction ends the search.
// A position inside an earlier window is skipped as :936-952 does; one that fails fracmv_within_tile costs 2^32 - 1 and
// never wins.  Result (all threads must call; ends with the values in sh, NOT yet visible: the caller synchronises).
template <bool CONSTR, bool QSAD, int T>
__device__ __forceinline__ void full_search_wg(int tid, u8 *lds, int lds_bytes, me_shared *sh, const u8 *__restrict__ pic, u32 pic_stride,
                                               const refplane_t &ref, const kvz_hip_me_pu &pu, const kvz_hip_me_params &prm)
{
  const me_cost_model_t<false, CONSTR> mvc(pu, prm);
  const int w = pu.width, h = pu.height, R = prm.search_range, side = 2 * R + 1;
  const int wq = w >> 2;                               // every PU width is a multiple of 4
  // ---- the windows, in the reference's order: sh->cx / cy = centre, sh->sad = index of the merge candidate (or -1) ----
  int n_win = 1;
  auto add_window = [&](int cx, int cy, int merge_index) {
    if (tid == 0) { sh->cx[n_win] = cx; sh->cy[n_win] = cy; sh->sad[n_win] = (u32)merge_index; }
    ++n_win;
  };
  if (tid == 0) { sh->cx[0] = 0; sh->cy[0] = 0; sh->sad[0] = ~0u; }
  {
    const int ex = pu.extra_mv[0] >> 2, ey = pu.extra_mv[1] >> 2;
    // (an extra window on the zero vector repeats window 0 and can improve nothing: costs must be strictly smaller)
    if (!mvc.in_merge(ex, ey) && (ex != 0 || ey != 0)) add_window(ex, ey, -1);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if (!(mvc.usable >> i & 1u)) continue;
      const int cx0 = mvc.mx[i] >> 2, cy0 = mvc.my[i] >> 2;        // plain shift here (:917-920)
      if (cx0 == 0 && cy0 == 0) continue;
      add_window(cx0, cy0, i);
    }
  }
  // ---- the current block never enters LDS: its address is the same in every lane, so it is read with scalar loads (constant address
  // space: s_load_dwordx2..x16 per row) and feeds the SAD instructions as SGPR operands.  The scalar cache may hold what a previous
  // unit of a resident worker read from a slot that has been overwritten since: dropped here.
  __builtin_amdgcn_s_dcache_inv();
  typedef const u32 __attribute__((address_space(4))) cu32;
  const cu32 *const cur_c = (const cu32 *)(unsigned long long)(pic + (size_t)pu.y * pic_stride + pu.x);     // 4-byte aligned: x and the stride are multiples of 4
  const int cstride = (int)(pic_stride >> 2);
  u8 *const s_win = lds;
  // an item is NQ quads of neighbouring positions of one window row: 4 positions when the windows give the 512 threads one round of
  // items or less, 8 otherwise (one more reference dword per row serves four more positions: half the LDS traffic per position)
  const int groups4 = (side + 3) >> 2, groups8 = (side + 7) >> 3;
  // (blocks up to 16 pixels wide are bound by the pricing of the positions, not by LDS: there 8 positions per item only pay when they
  // save rounds outright -- an item of two quads costs about 1.6 items of one)
  const int rounds4 = (n_win * side * groups4 + T - 1) / T, rounds8 = (n_win * side * groups8 + T - 1) / T;
  const bool wide = wq >= 8 ? rounds4 > 1 : 16 * rounds8 < 10 * rounds4;
  const int groups = wide ? groups8 : groups4;
  const int wstride = (w + 8 * groups8 + 4 + 3) & ~3, wrows = h + 2 * R, win_bytes = wstride * wrows, wsq = wstride >> 2;
  int per_chunk = lds_bytes / win_bytes;                // >= 1 for every legal PU and range (64x64, R = 64: 204 x 192 bytes)
  if (per_chunk > FULL_MAX_WINDOWS) per_chunk = FULL_MAX_WINDOWS;
  const int items_per_win = side * groups;
  unsigned long long best = ~0ull;
  __syncthreads();                                      // the window list

  // prices the positions of one quad of an item and keeps the thread's smallest (cost, visiting order)
  auto price_quad = [&](int kk, int r, int col0, const u32 (&tot)[4]) {
    const int cx = sh->cx[kk], cy = sh->cy[kk], mine = (int)sh->sad[kk];
    const int y = cy + r - R;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int col = col0 + p, x = cx + col - R;
      if (col >= side) continue;
      bool skip = false;
      if (mine >= 0) {                                   // a merge candidate's window: :936-952
        if (x >= -R && x <= R && y >= -R && y <= R) skip = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= mine || !(mvc.usable >> j & 1u)) continue;
          const int xx = mvc.mx[j] >> 2, yy = mvc.my[j] >> 2;
          if (x >= xx - R && x <= xx + R && y >= yy - R && y <= yy + R) skip = true;
        }
      }
      if (skip || !mvc.within(x * 4, y * 4)) continue;
      u32 bits;
      const u32 cost = tot[p] + mvc.cost(x, y, 2, bits);                  // < 2^32: lambda_cost is bounded by the entry
      const unsigned long long key = ((unsigned long long)cost << 32) | (u32)(kk * side * side + r * side + col);
      best = key < best ? key : best;
    }
  };
  // the SADs of an item: WQ = dwords per block row (0: any width, one scalar load per dword), NQ = quads
  auto run_items = [&](auto wq_tag, auto nq_tag, int k0, int nk) {
    constexpr int WQ = decltype(wq_tag)::value, NQ = decltype(nq_tag)::value;
    const int nwq = WQ ? WQ : wq;
    const int flush_rows = nwq >= 64 ? 1 : 64 / nwq;    // rows of 16-bit sums that cannot overflow: 64 x 4 x 255 < 2^16
    for (int it = tid; it < nk * items_per_win; it += T) {
      const int k = it / items_per_win, rem = it - k * items_per_win, r = rem / groups, g = rem - r * groups;
      const u32 *q = (const u32 *)(s_win + k * win_bytes + r * wstride) + NQ * g;
      const cu32 *c = cur_c;
      u32 tot[NQ][4] = {};
      for (int yb = 0; yb < h; yb += flush_rows) {
        const int ye = yb + flush_rows < h ? yb + flush_rows : h;
        unsigned long long acc[NQ] = {};
        for (int y = yb; y < ye; ++y) {
          u32 d[NQ + 1];
#pragma unroll
          for (int i = 0; i < NQ; ++i) d[i] = q[i];
#pragma unroll 16
          for (int xq = 0; xq < nwq; ++xq) {
            d[NQ] = q[xq + NQ];
            const u32 cv = c[xq];
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
              if (QSAD) {
                acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(((unsigned long long)d[i + 1] << 32) | d[i], cv, acc[i]);
              } else {
                tot[i][0] = __builtin_amdgcn_sad_u8(cv, d[i], tot[i][0]);
                tot[i][1] = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(d[i + 1], d[i], 1u), tot[i][1]);
                tot[i][2] = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(d[i + 1], d[i], 2u), tot[i][2]);
                tot[i][3] = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(d[i + 1], d[i], 3u), tot[i][3]);
              }
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i) d[i] = d[i + 1];
          }
          q += wsq; c += cstride;
        }
        if (QSAD) {
#pragma unroll
          for (int i = 0; i < NQ; ++i) {
            tot[i][0] += (u32)acc[i] & 0xffffu; tot[i][1] += (u32)(acc[i] >> 16) & 0xffffu;
            tot[i][2] += (u32)(acc[i] >> 32) & 0xffffu; tot[i][3] += (u32)(acc[i] >> 48);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NQ; ++i) price_quad(k0 + k, r, 4 * (NQ * g + i), tot[i]);
    }
  };
  auto run_width = [&](auto nq_tag, int k0, int nk) {
    switch (wq) {
      case 2: run_items(std::integral_constant<int, 2>(), nq_tag, k0, nk); break;
      case 4: run_items(std::integral_constant<int, 4>(), nq_tag, k0, nk); break;
      case 8: run_items(std::integral_constant<int, 8>(), nq_tag, k0, nk); break;
      case 16: run_items(std::integral_constant<int, 16>(), nq_tag, k0, nk); break;
      default: run_items(std::integral_constant<int, 0>(), nq_tag, k0, nk); break;
    }
  };

  for (int k0 = 0; k0 < n_win; k0 += per_chunk) {
    const int nk = n_win - k0 < per_chunk ? n_win - k0 : per_chunk;
    if (k0) __syncthreads();                            // the previous chunk has been read
    for (int k = 0; k < nk; ++k) {
      const int x0 = pu.x + sh->cx[k0 + k] - R, y0 = pu.y + sh->cy[k0 + k] - R;
      u8 *const dst = s_win + k * win_bytes;
      for (int i = tid; i < wsq * wrows; i += T) {
        const int y = i / wsq, q = (i - y * wsq) * 4;
        u32 v;
        if (x0 + q >= 0 && x0 + q + 4 <= ref.w && y0 + y >= 0 && y0 + y < ref.h) {
          __builtin_memcpy(&v, ref.p + (size_t)(y0 + y) * ref.stride + x0 + q, 4);
        } else {
          v = (u32)ref_px(ref, x0 + q, y0 + y) | ((u32)ref_px(ref, x0 + q + 1, y0 + y) << 8) |
              ((u32)ref_px(ref, x0 + q + 2, y0 + y) << 16) | ((u32)ref_px(ref, x0 + q + 3, y0 + y) << 24);
        }
        *(u32 *)(dst + y * wstride + q) = v;
      }
    }
    __syncthreads();
    if (wide) run_width(std::integral_constant<int, 2>(), k0, nk);
    else run_width(std::integral_constant<int, 1>(), k0, nk);
  }
  // ---- the smallest (cost, order) of the workgroup ----
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u32 lo = (u32)__shfl_xor((int)(u32)best, off, 64), hi = (u32)__shfl_xor((int)(u32)(best >> 32), off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    best = o < best ? o : best;
  }
  __syncthreads();                                      // every reader of the window list is done; sh->sad is reused
  if ((tid & 63) == 0) { sh->sad[48 + 2 * (tid >> 6)] = (u32)best; sh->sad[49 + 2 * (tid >> 6)] = (u32)(best >> 32); }
  __syncthreads();
  best = ~0ull;
#pragma unroll
  for (int v = 0; v < T / 64; ++v) {
    const unsigned long long o = ((unsigned long long)sh->sad[49 + 2 * v] << 32) | sh->sad[48 + 2 * v];
    best = o < best ? o : best;
  }
  if (tid == 0) {
    int bx = 0, by = 0;
    u32 bcost = 0xffffffffu, bbits = 0;
    if ((u32)(best >> 32) != 0xffffffffu) {
      const int seq = (int)(u32)best, kk = seq / (side * side), rem = seq - kk * side * side, r = rem / side, col = rem - r * side;
      bx = sh->cx[kk] + col - R; by = sh->cy[kk] + r - R;
      bcost = (u32)(best >> 32);
      mvc.cost(bx, by, 2, bbits);
    }
    sh->cx[FULL_OUT] = bx; sh->cy[FULL_OUT] = by; sh->sad[FULL_OUT] = bcost; sh->sad[FULL_OUT + 1] = bbits;
  }
}

// One PU.  T threads (a wave with wave-private LDS, or the whole workgroup) share the work; every thread
// carries the same search state, so all decisions are uniform across them.
// BOTH (the search service, serve.hip): the fractional stage always runs and `out` is a serve_result that also receives the
// outcome search_pu_inter_ref reaches when the integer search does not beat *inter_cost (:1239-1252), so that the pictures
// of a PU can be searched in parallel and the sequential rule replayed afterwards.
template <int MAXW, int T, bool WAVE, int FW = 0, int FH = 0, bool RDO = false, bool CONSTR = true, bool BOTH = false>
__device__ __forceinline__ void search_pu_core(int tid, u8 *lds, me_shared *sh, const u8 *__restrict__ pic, u32 pic_stride,
                                               const refplane_t &ref, const kvz_hip_me_pu &pu, const kvz_hip_me_params &prm,
                                               kvz_hip_me_result *__restrict__ out, size_t pu_index)
{
  typedef frac_geom<MAXW> G;
  u8 *s_cur = lds + G::P_BYTES;                        // same place search_frac_core keeps the current block
  auto sync = [&]() { if (WAVE) wave_lds_fence(); else __syncthreads(); };
  const me_cost_model_t<RDO, CONSTR> mvc(pu, prm);
  const int w = FW ? FW : pu.width, h = FH ? FH : pu.height;                       // FW, FH: compile-time size (0 = runtime)
  // a row is cut into 8-pixel segments, or 4-pixel ones when the width is 4 or 12 (AMP / SMP shapes)
  const bool seg4 = !FW && (w & 4);
  const int segw = seg4 ? 4 : 8, w8 = seg4 ? w >> 2 : w >> 3, segs = w8 * h;       // w8: segments per row

  for (int i = tid; i < segs; i += T) {
    const int y = i / w8, x = (i - y * w8) * segw;
    if (seg4) {
      u32 v;
      __builtin_memcpy(&v, pic + (size_t)(pu.y + y) * pic_stride + pu.x + x, 4);
      *(u32 *)(s_cur + y * G::CS + x) = v;
    } else {
      uint2 v;
      __builtin_memcpy(&v, pic + (size_t)(pu.y + y) * pic_stride + pu.x + x, 8);
      *(uint2 *)(s_cur + y * G::CS + x) = v;
    }
  }

  int best_x = 0, best_y = 0;                          // info->best_mv, integer-pel here
  u32 best_cost = 0xffffffffu, best_bits = 0;

  // Exhaustive search only: the reference pixels of one (2R+1)^2 window, staged in LDS behind the current block
  // (the fractional stage's buffers are idle until the integer search is over) when they fit.
  u8 *const s_win = lds + G::P_BYTES + G::CUR_BYTES;
  constexpr int WIN_BYTES = G::TOTAL - (G::P_BYTES + G::CUR_BYTES);
  int win_cx = 0, win_cy = 0, win_R = 0, win_stride = 0;
  bool win_on = false;

  const bool seg_pow2 = (segs & (segs - 1)) == 0 && segs >= 8;
  const int run = segs < 64 ? segs : 64;

  // SADs of candidates 0 .. n-1 (offsets in sh->cx / cy, written by the caller) -> sh->sad
  auto group_sads = [&](int n) {
    if (tid < ME_GROUP) sh->sad[tid] = 0;
    sync();
    if (win_on) {
      // Exhaustive search, window in LDS: ONE LANE PER POSITION walks the block's row segments (the current block's
      // segment is the same address for every lane: an LDS broadcast), so a position's SAD never leaves its lane -- no
      // per-item index arithmetic, no cross-lane reduction, no atomics for a one-wave PU.  Wider workgroups split the
      // segments between their waves.
      const int k = tid & (ME_GROUP - 1), part = tid / ME_GROUP, nparts = T / ME_GROUP;
      if (k < n) {
        const int col0 = sh->cx[k] - win_cx + win_R, row0 = sh->cy[k] - win_cy + win_R;
        u32 acc = 0;
        for (int s = part; s < segs; s += nparts) {
          const int y = s / w8, x = (s - y * w8) * segw;
          const int col = col0 + x;
          const u32 *q = (const u32 *)(s_win + (row0 + y) * win_stride + (col & ~3));
          const u32 sh8 = (u32)col & 3u;
          if (seg4) {
            acc = __builtin_amdgcn_sad_u8(*(const u32 *)(s_cur + y * G::CS + x), __builtin_amdgcn_alignbyte(q[1], q[0], sh8), acc);
          } else {
            const uint2 c = *(const uint2 *)(s_cur + y * G::CS + x);
            const u32 d0 = q[0], d1 = q[1], d2 = q[2];
            acc = __builtin_amdgcn_sad_u8(c.x, __builtin_amdgcn_alignbyte(d1, d0, sh8), acc);
            acc = __builtin_amdgcn_sad_u8(c.y, __builtin_amdgcn_alignbyte(d2, d1, sh8), acc);
          }
        }
        if (nparts == 1) sh->sad[k] = acc; else atomicAdd(&sh->sad[k], acc);
      }
      sync();
      return;
    }
    for (int it = tid; it < n * segs; it += T) {
      const int k = it / segs, s = it - k * segs, y = s / w8, x = (s - y * w8) * segw;
      uint2 c, r;
      if (seg4) {
        c.x = *(const u32 *)(s_cur + y * G::CS + x); c.y = 0u; r.y = 0u;
        const int rx = pu.x + sh->cx[k] + x, ry = pu.y + sh->cy[k] + y;
        if (rx >= 0 && rx + 4 <= ref.w && ry >= 0 && ry < ref.h) {
          __builtin_memcpy(&r.x, ref.p + (size_t)ry * ref.stride + rx, 4);
        } else {
          r.x = (u32)ref_px(ref, rx, ry) | ((u32)ref_px(ref, rx + 1, ry) << 8) | ((u32)ref_px(ref, rx + 2, ry) << 16) |
                ((u32)ref_px(ref, rx + 3, ry) << 24);
        }
      } else {
        c = *(const uint2 *)(s_cur + y * G::CS + x);
        const int rx = pu.x + sh->cx[k] + x, ry = pu.y + sh->cy[k] + y;
        if (rx >= 0 && rx + 8 <= ref.w && ry >= 0 && ry < ref.h) {
          __builtin_memcpy(&r, ref.p + (size_t)ry * ref.stride + rx, 8);
        } else {
          u32 b[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) b[i] = ref_px(ref, rx + i, ry);
          r.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
          r.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        }
      }
      u32 v = __builtin_amdgcn_sad_u8(c.y, r.y, __builtin_amdgcn_sad_u8(c.x, r.x, 0u));
      if (seg_pow2) {
        // the lanes that share a candidate are an aligned run of min(segs, 64): add them up in registers first --
        // 32 lanes hitting one LDS address with an atomic serialise
        v = run == 8 ? group_sum<8>(v) : run == 16 ? group_sum<16>(v) : run == 32 ? group_sum<32>(v) : group_sum<64>(v);   // DPP up to 16 lanes
        if (((tid & 63) & (run - 1)) == 0) atomicAdd(&sh->sad[k], v);
      } else {
        atomicAdd(&sh->sad[k], v);
      }
    }
    sync();
  };
  // check_mv_cost (:195-232) over the evaluated group at once.  The reference walks the candidates in order and
  // replaces the best on a strictly smaller cost, i.e. it ends on the FIRST candidate that attains the group's minimum,
  // provided that minimum beats the incoming best -- and that candidate is also the last one that "improved", which is
  // what the patterns record as best_index.  Lane k prices candidate k; a wave-wide minimum and a ballot pick the
  // same winner.  Returns its index in the group, or -1 when nothing improved.  (Every wave of a workgroup computes
  // this redundantly from the same LDS values, so the result is uniform without another barrier.)
  auto decide = [&](int n) -> int {
    const int k = tid & 63;
    u32 cost = 0xffffffffu, bits = 0;
    int x = 0, y = 0;
    if (k < n) {
      x = sh->cx[k]; y = sh->cy[k];
      if (mvc.within(x * 4, y * 4)) cost = sh->sad[k] + mvc.cost(x, y, 2, bits);   // < 2^32: lambda_cost is bounded by the entry
    }
    u32 m = cost;
    if (n <= 16) {
      // every pattern but the exhaustive search: the candidates sit in lanes 0..15, one DPP row -- four v_min with
      // DPP operands instead of six LDS-crossbar exchanges
      u32 o;
      o = dpp_mov<0xB1>(m); m = o < m ? o : m;             // quad_perm [1,0,3,2]
      o = dpp_mov<0x4E>(m); m = o < m ? o : m;             // quad_perm [2,3,0,1]
      o = dpp_mov<0x141>(m); m = o < m ? o : m;            // row_half_mirror
      o = dpp_mov<0x140>(m); m = o < m ? o : m;            // row_mirror
      m = (u32)__builtin_amdgcn_readfirstlane((int)m);
    } else {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const u32 o = (u32)__shfl_xor((int)m, off, 64);
        m = o < m ? o : m;
      }
    }
    if (m >= best_cost) return -1;
    const int win = __builtin_ctzll(__ballot(cost == m));
    best_x = __shfl(x, win, 64); best_y = __shfl(y, win, 64);
    best_cost = m; best_bits = (u32)__shfl((int)bits, win, 64);
    return win;
  };
  auto set_cand = [&](int k, int x, int y) { if (tid == 0) { sh->cx[k] = x; sh->cy[k] = y; } };

  bool done = false;
  if (BOTH && prm.algorithm == 3) {
    // the search service: the whole workgroup has already walked the windows (full_search_wg, above); its outcome waits in sh
    best_x = sh->cx[FULL_OUT]; best_y = sh->cy[FULL_OUT];
    best_cost = sh->sad[FULL_OUT]; best_bits = sh->sad[FULL_OUT + 1];
    done = true;
  } else if (prm.algorithm == 3) {
    // ---- search_mv_full (:886-962): the windows around the zero vector, extra_mv and the merge candidates, in the
    // reference's visiting order, ME_GROUP positions per round ----
    const int R = prm.search_range;
    int n = 0;
    sync();
    auto flush = [&]() {
      if (n > 0) {
        group_sads(n);
        decide(n);
        n = 0;
        sync();
      }
    };
    auto push = [&](int x, int y) {
      set_cand(n++, x, y);
      if (n == ME_GROUP) flush();
    };
    // a window's (w + 2R) x (h + 2R) reference pixels (edge replicated, image.c:320-444) go to LDS when they fit
    auto begin_window = [&](int cx, int cy) {
      flush();
      const int stride = ((w + 2 * R + 3) & ~3) + 4, rows = h + 2 * R;
      win_on = stride * rows <= WIN_BYTES;
      if (win_on) {
        win_cx = cx; win_cy = cy; win_R = R; win_stride = stride;
        const int x0 = pu.x + cx - R, y0 = pu.y + cy - R, wq = stride >> 2;
        for (int i = tid; i < wq * rows; i += T) {
          const int y = i / wq, q = (i - y * wq) * 4;
          u32 v;
          if (x0 + q >= 0 && x0 + q + 4 <= ref.w && y0 + y >= 0 && y0 + y < ref.h) {
            __builtin_memcpy(&v, ref.p + (size_t)(y0 + y) * ref.stride + x0 + q, 4);
          } else {
            v = (u32)ref_px(ref, x0 + q, y0 + y) | ((u32)ref_px(ref, x0 + q + 1, y0 + y) << 8) |
                ((u32)ref_px(ref, x0 + q + 2, y0 + y) << 16) | ((u32)ref_px(ref, x0 + q + 3, y0 + y) << 24);
          }
          *(u32 *)(s_win + y * stride + q) = v;
        }
        sync();
      }
    };
    begin_window(0, 0);
    for (int y = -R; y <= R; ++y)
      for (int x = -R; x <= R; ++x) push(x, y);
    const int ex = pu.extra_mv[0] >> 2, ey = pu.extra_mv[1] >> 2;
    if (!mvc.in_merge(ex, ey)) {
      begin_window(ex, ey);
      for (int y = -R; y <= R; ++y)
        for (int x = -R; x <= R; ++x) push(ex + x, ey + y);
    }
#pragma unroll                                              // i and j are unrolled so that mx[] / my[] stay in registers
    for (int i = 0; i < 5; ++i) {
      if (!(mvc.usable >> i & 1u)) continue;
      const int cx0 = mvc.mx[i] >> 2, cy0 = mvc.my[i] >> 2;        // plain shift here (:917-920)
      if (cx0 == 0 && cy0 == 0) continue;
      begin_window(cx0, cy0);
      for (int y = cy0 - R; y <= cy0 + R; ++y)
        for (int x = cx0 - R; x <= cx0 + R; ++x) {
          if (!mvc.within(x * 4, y * 4)) continue;
          bool tested = false;
#pragma unroll
          for (int j = -1; j < 4; ++j) {
            if (j >= i || tested) continue;
            int xx = 0, yy = 0;
            if (j >= 0) {
              if (!(mvc.usable >> j & 1u)) continue;
              xx = mvc.mx[j >= 0 ? j : 0] >> 2; yy = mvc.my[j >= 0 ? j : 0] >> 2;
            }
            if (x >= xx - R && x <= xx + R && y >= yy - R && y <= yy + R) {
              tested = true;
              x = xx + R;                                          // jump past the earlier window (:948)
            }
          }
          if (!tested) push(x, y);
        }
    }
    flush();
    win_on = false;
    done = true;
  }

  // ---- select_starting_point (:282-307) ----
  int n = 0;
  sync();                                              // s_cur complete; previous readers of sh are done
  if (!done) {
  set_cand(n++, 0, 0);
  {
    const int ex = pu.extra_mv[0] >> 2, ey = pu.extra_mv[1] >> 2;
    if ((ex != 0 || ey != 0) && !mvc.in_merge(ex, ey)) set_cand(n++, ex, ey);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if (!(mvc.usable >> i & 1u)) continue;
      const int x = (mvc.mx[i] + 2) >> 2, y = (mvc.my[i] + 2) >> 2;
      if (x == 0 && y == 0) continue;
      set_cand(n++, x, y);
    }
  }
  group_sads(n);
  decide(n);
  }

  // ---- early_terminate (:415-460) ----
  if (!done && prm.early_termination) {
    int mvx = best_x, mvy = best_y, first = 0, last = 3;
    for (int round = 0; round < 2 && !done; ++round) {
      const double threshold = prm.early_termination == 2 ? (double)best_cost * 0.95 : (double)best_cost;
      sync();
      for (int i = first; i <= last; ++i) set_cand(i - first, mvx + c_et_hex[i][0], mvy + c_et_hex[i][1]);
      group_sads(last - first + 1);
      const int hit = decide(last - first + 1);
      const int best_index = hit >= 0 ? first + hit : 6;
      mvx += c_et_hex[best_index][0]; mvy += c_et_hex[best_index][1];
      if ((double)best_cost >= threshold) done = true;
      first = (best_index + 3) % 4;
      last = first + 2;
    }
  }

  if (!done && prm.algorithm == 2) {
    // ---- tz_search (:595-672): search range 96, 8-point diamond patterns (4 points at distance 1), no raster
    // scan, star refinement; kvz_tz_pattern_search (:463-577) is one group ----
    int best_dist = 0;
    auto pattern = [&](int dist, int sx, int sy) {
      const int hd = dist / 2, n = dist == 1 ? 4 : 8;
      sync();
      set_cand(0, sx, sy + dist); set_cand(1, sx + dist, sy); set_cand(2, sx, sy - dist); set_cand(3, sx - dist, sy);
      if (n == 8) {
        set_cand(4, sx + hd, sy + hd); set_cand(5, sx + hd, sy - hd); set_cand(6, sx - hd, sy - hd); set_cand(7, sx - hd, sy + hd);
      }
      group_sads(n);
      if (decide(n) >= 0) best_dist = dist;
    };
    int sx = best_x, sy = best_y, rounds = 0;
    for (int dist = 1; dist <= 96; dist *= 2) {
      pattern(dist, sx, sy);
      if (best_dist != dist) rounds++;
      if (rounds >= 3) break;
    }
    if (sx != 0 || sy != 0) {
      rounds = 0;
      for (int dist = 1; dist <= 48; dist *= 2) {
        pattern(dist, 0, 0);
        if (best_dist != dist) rounds++;
        if (rounds >= 3) break;
      }
    }
    while (best_dist > 0) {
      best_dist = 0;
      sx = best_x; sy = best_y;
      for (int dist = 1; dist <= 96; dist *= 2) pattern(dist, sx, sy);
    }
  } else if (!done && prm.algorithm == 1) {
    // ---- diamond_search (:826-882) ----
    int mvx = best_x, mvy = best_y, best_index = 4;
    u32 steps = prm.max_steps;
    sync();
    for (int i = 0; i < 5; ++i) set_cand(i, mvx + c_diamond[i][0], mvy + c_diamond[i][1]);
    group_sads(5);
    {
      const int hit = decide(5);
      if (hit >= 0) best_index = hit;
    }
    if (best_index != 4) {
      mvx += c_diamond[best_index][0]; mvy += c_diamond[best_index][1];
      int from_dir = 4;
      bool better;
      do {
        better = false;
        if (steps > 0) steps -= 1;
        sync();
        int n = 0, idx[4];
        for (int i = 0; i < 4; ++i) {
          if (i == from_dir) continue;                  // where we came from is checked already
          idx[n] = i;
          set_cand(n++, mvx + c_diamond[i][0], mvy + c_diamond[i][1]);
        }
        group_sads(n);
        const int hit = decide(n);
        if (hit >= 0) { best_index = hit == 0 ? idx[0] : (hit == 1 ? idx[1] : (hit == 2 ? idx[2] : idx[3])); better = true; }
        if (better) {
          mvx += c_diamond[best_index][0]; mvy += c_diamond[best_index][1];
          from_dir = best_index ^ 3;
        }
      } while (better && steps != 0);
    }
  } else if (!done) {
    // ---- the hexagon (:723-777) ----
    int mvx = best_x, mvy = best_y, best_index = 0;
    u32 steps = prm.max_steps;
    sync();
    for (int i = 1; i < 7; ++i) set_cand(i - 1, mvx + c_large_hex[i][0], mvy + c_large_hex[i][1]);
    group_sads(6);
    {
      const int hit = decide(6);
      if (hit >= 0) best_index = hit + 1;
    }
    while (best_index != 0 && steps != 0) {
      steps -= 1;
      const int start = best_index == 1 ? 6 : (best_index == 8 ? 1 : best_index - 1);
      mvx += c_large_hex[best_index][0]; mvy += c_large_hex[best_index][1];
      best_index = 0;
      sync();
      for (int i = 0; i < 3; ++i) set_cand(i, mvx + c_large_hex[start + i][0], mvy + c_large_hex[start + i][1]);
      group_sads(3);
      const int hit = decide(3);
      if (hit >= 0) best_index = start + hit;
    }
    sync();
    for (int i = 1; i < 9; ++i) set_cand(i - 1, mvx + c_small_hex[i][0], mvy + c_small_hex[i][1]);
    group_sads(8);
    decide(8);
  }

  // ---- search_frac, or the SATD re-cost of :1236-1248 when cfg.fme_level == 0 ----
  int mv_x = best_x * 4, mv_y = best_y * 4;
  const u32 int_cost = best_cost, int_bits = best_bits;
  u32 cost0 = 0xffffffffu;
  if (best_cost != 0xffffffffu) {
    sync();
    const kvz_hip_block_pair d = { pu.x, pu.y, pu.x + best_x, pu.y + best_y, w, h };
    // :1239: the fractional search only if the integer result beats what the pictures searched before reached
    const u32 beat = (!BOTH && prm.cost_to_beat) ? prm.cost_to_beat[pu_index] : 0xffffffffu;
    const int level = __builtin_amdgcn_readfirstlane(best_cost < beat ? prm.fme_level : 0);   // the same in every lane: keep the level's branches scalar
    const frac_result fr = search_frac_core<MAXW, T, WAVE, me_cost_model_t<RDO, CONSTR>, FW, FH>(tid, lds, pic, pic_stride, ref, d, level, mvc, (u32 *)nullptr, (i32 *)nullptr);
    best_cost = fr.cost;                               // level 0: satd + bits(int mv) * lambda, the same bits as best_bits
    cost0 = fr.cost0;
    if (level > 0) { mv_x = fr.mvx; mv_y = fr.mvy; best_bits = fr.bitcost; }
  }

  if (BOTH) {
    if (tid == 0) {
      serve_result *so = reinterpret_cast<serve_result *>(out);
      kvz_hip_me_result r;
      u32 unused;
      r.mv[0] = mv_x; r.mv[1] = mv_y;
      r.cost = best_cost; r.bitcost = best_bits;
      int m = mvc.merge_match(mv_x, mv_y);
      r.merged = m >= 0;
      r.merge_idx = m >= 0 ? m : mvc.n_merge;
      r.mv_cand = m >= 0 ? 0 : mvc.select_cand(mv_x, mv_y, unused);
      r.reserved = 0;
      so->frac = r;
      r.mv[0] = best_x * 4; r.mv[1] = best_y * 4;          // :1242-1252: the integer vector, SATD + its bits
      r.cost = cost0; r.bitcost = int_bits;
      m = mvc.merge_match(best_x * 4, best_y * 4);
      r.merged = m >= 0;
      r.merge_idx = m >= 0 ? m : mvc.n_merge;
      r.mv_cand = m >= 0 ? 0 : mvc.select_cand(best_x * 4, best_y * 4, unused);
      so->integer = r;
      so->integer_search_cost = int_cost;
      // the caller polls `done` in page-locked host memory: results first, system-wide, then the flag
      __threadfence_system();
      __hip_atomic_store(&so->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  if (tid == 0) {
    kvz_hip_me_result r;
    r.mv[0] = mv_x; r.mv[1] = mv_y;
    r.cost = best_cost; r.bitcost = best_bits;
    const int m = mvc.merge_match(mv_x, mv_y);          // :1253-1266
    r.merged = m >= 0;
    r.merge_idx = m >= 0 ? m : mvc.n_merge;
    u32 unused;
    r.mv_cand = m >= 0 ? 0 : (RDO ? mvc.select_cand_cabac(mv_x, mv_y) : mvc.select_cand(mv_x, mv_y, unused));   // :1268-1273
    r.reserved = 0;
    *out = r;
  }
}

__device__ __forceinline__ bool pu_ok(const kvz_hip_me_pu &pu, int pic_w, int pic_h)
{
  return frac_shape_ok(pu.width, pu.height) && pu.x >= 0 && pu.y >= 0 && pu.x + pu.width <= pic_w && pu.y + pu.height <= pic_h &&
         pu.num_merge_cand >= 0 && pu.num_merge_cand <= 5;
}

__device__ __forceinline__ void flag_bad(kvz_hip_me_result *out)
{
  kvz_hip_me_result r = { { 0, 0 }, 0xffffffffu, 0, 0, 0, 0, -1 };
  *out = r;
}

// size class of a PU as kvz_hip_me_params.size_classes names them: 1 = up to 16x16, 2 = up to 32x32, 4 = larger
__device__ __forceinline__ int pu_class(const kvz_hip_me_pu &pu)
{
  return (pu.width > 32 || pu.height > 32) ? 4 : ((pu.width > 16 || pu.height > 16) ? 2 : 1);
}
// A launch with a size-class hint starts only the kernels of the classes named, so a PU of another class is searched by
// no kernel: the kernel of the lowest class named flags it (cost 0xFFFFFFFF, reserved -1) on its way past.
__device__ __forceinline__ bool pu_orphan(int cls, int mine, int hinted) { return !(hinted & cls) && mine == (hinted & -hinted); }

}  // namespace kvzhip

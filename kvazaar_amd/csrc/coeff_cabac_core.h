// coeff_cabac_core.h -- the reference's CABAC price of one TU's coefficients: what get_coeff_cabac_cost (rdo.c:158-197) returns, the bits
// that kvz_encode_coeff_nxn (encode_coding_tree.c:103-345, with encode_last_significant_xy :49-101) produces in counting mode from a
// given `range` and context set.  The count (23 - bits_left) + 8 * num_buffered_bytes is the number of renormalisation shifts plus the
// number of bypass bins (cabac.c:91-256: kvz_cabac_write only moves eight of them from one counter to the other), so `low` is not kept.
//
// coeff_cabac_count is the serial recursion over (range, context states), run by ONE lane.  What it reads is handed in by two small
// accessors, so that the callers decide where a TU and its private context set live:
//   Coeffs: int at(int x, int y) const     -- the coefficient at column x, row y
//   Ctx:    u32 get(int i) const, void set(int i, u32 v)   -- the caller's COPY of kvz_hip_coeff_ctx.ctx, i in 0..137
// Neither is indexed with anything but values derived from the TU's geometry, and a context byte is masked before it indexes a table,
// so no coefficient and no context value can cause an access outside a table.  The crypto branches of the reference are not reached
// in counting mode.  coeff_cost.hip holds the batch entry's kernels; the _ts_cabac stages price their trials with the same function.
#pragma once
#include "cabac_tables.h"

namespace kvzhip {

// kvz_hip_coeff_ctx.ctx: cabac_data_t.ctx from cu_sig_coeff_group_model[0] on (cabac.h:65-75), then the two transform_skip models
enum : int {
  CC_SIG_CG = 0, CC_SIG_LUMA = 4, CC_SIG_CHROMA = 31, CC_LAST_Y_LUMA = 46, CC_LAST_Y_CHROMA = 61, CC_LAST_X_LUMA = 76, CC_LAST_X_CHROMA = 91,
  CC_ONE_LUMA = 106, CC_ONE_CHROMA = 122, CC_ABS_LUMA = 130, CC_ABS_CHROMA = 134, CC_TS_LUMA = 136, CC_TS_CHROMA = 137, CC_CTX_USED = 138
};

// The scans as x | y << 4: the 16 positions of a 4x4 group per scan mode (kvz_g_sig_last_scan[mode][1], tables.c:15-17) and the
// coefficient groups of a TU of 2, 4 or 8 groups a side (g_sig_last_scan_cg, tables.h:37-77; modes 1 / 2 exist for 2 a side only).
// A TU's scan is its groups in group order, each in the 4x4 order of the mode.
struct cc_scans { u8 inner[3][16]; u8 cg2[3][4]; u8 cg4[16]; u8 cg8[64]; };
constexpr void cc_fill_scan(u8 *out, int n, int mode)
{
  int k = 0;
  if (mode == 1) { for (int y = 0; y < n; ++y) for (int x = 0; x < n; ++x) out[k++] = (u8)(x | y << 4); }
  else if (mode == 2) { for (int x = 0; x < n; ++x) for (int y = 0; y < n; ++y) out[k++] = (u8)(x | y << 4); }
  else {
    for (int d = 0; d < 2 * n - 1; ++d)                  // up-right diagonals, each from its lower-left end
      for (int y = d < n ? d : n - 1; y >= 0 && d - y < n; --y) out[k++] = (u8)((d - y) | y << 4);
  }
}
constexpr cc_scans cc_make_scans()
{
  cc_scans s = {};
  for (int m = 0; m < 3; ++m) { cc_fill_scan(s.inner[m], 4, m); cc_fill_scan(s.cg2[m], 2, m); }
  cc_fill_scan(s.cg4, 4, 0);
  cc_fill_scan(s.cg8, 8, 0);
  return s;
}
static __constant__ cc_scans c_cc_scans = cc_make_scans();
static __constant__ u8 c_cc_group_idx[32] = { 0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9 };   // encoderstate.h:345
static __constant__ u8 c_cc_sig_4x4[16] = { 0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8, 8 };                  // ctx_ind_map, context.c:357

struct coeff_cabac_flags { bool signhide, trskip_enable, lossless; };

template <class Ctx>
struct coeff_coder {
  Ctx ctx;
  u32 range, bits;
  __device__ __forceinline__ void bin(int i, u32 b)            // kvz_cabac_encode_bin, cabac.c:91-120
  {
    const u32 uc = ctx.get(i), st = (uc >> 1) & 63u, mps = uc & 1u, lps = c_range_lps[st * 4 + ((range >> 6) & 3u)];
    range -= lps;
    if (b != mps) {
      const u32 n = (u32)__clz((int)(lps >> 3)) - 26u;
      range = lps << n;
      bits += n;
      ctx.set(i, ((u32)c_trans_lps[st] << 1) | (mps ^ (st == 0 ? 1u : 0u)));
    } else {
      ctx.set(i, ((st < 62 ? st + 1 : st) << 1) | mps);
      if (range < 256) { range <<= 1; ++bits; }
    }
  }
  __device__ __forceinline__ void remain(u32 symbol, u32 r)    // kvz_cabac_write_coeff_remain, cabac.c:263-282: bypass bins only
  {
    if (symbol < (3u << r)) { bits += (symbol >> r) + 1 + r; return; }
    u32 length = r;
    symbol -= 3u << r;
    while (symbol >= (1u << length)) { symbol -= 1u << length; ++length; }
    bits += 3 + length + 1 - r + length;
  }
  __device__ __forceinline__ void last_xy(int x, int y, int log2w, int type, int scan_mode)   // encode_last_significant_xy
  {
    const int index = log2w - 2;
    const int ctx_offset = type ? 0 : index * 3 + (index + 1) / 4, shift = type ? index : (index + 3) / 4;
    const int base_x = (type ? CC_LAST_X_CHROMA : CC_LAST_X_LUMA) + ctx_offset, base_y = (type ? CC_LAST_Y_CHROMA : CC_LAST_Y_LUMA) + ctx_offset;
    if (scan_mode == 2) { const int t = x; x = y; y = t; }
    const int gx = c_cc_group_idx[x], gy = c_cc_group_idx[y], top = c_cc_group_idx[(1 << log2w) - 1];
    for (int k = 0; k < gx; ++k) bin(base_x + (k >> shift), 1);
    if (gx < top) bin(base_x + (gx >> shift), 0);
    for (int k = 0; k < gy; ++k) bin(base_y + (k >> shift), 1);
    if (gy < top) bin(base_y + (gy >> shift), 0);
    if (gx > 3) bits += (u32)(gx - 2) >> 1;
    if (gy > 3) bits += (u32)(gy - 2) >> 1;
  }
};

// kvz_context_get_sig_ctx_inc, context.c:354-385
__device__ __forceinline__ int cc_sig_ctx_inc(int pattern, int scan_mode, int x, int y, int log2w, int type)
{
  if (x + y == 0) return 0;
  if (log2w == 2) return c_cc_sig_4x4[4 * y + x];
  const int offset = log2w == 3 ? (scan_mode == 0 ? 9 : 15) : (type == 0 ? 21 : 12);
  const int xs = x & 3, ys = y & 3;
  int cnt;
  if (pattern == 0) cnt = xs + ys <= 2 ? (xs + ys == 0 ? 2 : 1) : 0;
  else if (pattern == 1) cnt = ys <= 1 ? (ys == 0 ? 2 : 1) : 0;
  else if (pattern == 2) cnt = xs <= 1 ? (xs == 0 ? 2 : 1) : 0;
  else cnt = 2;
  return ((type == 0 && ((x >> 2) + (y >> 2)) > 0) ? 3 : 0) + offset + cnt;
}

// Bits of one TU.  log2w 2..5, type 0 (luma) / 2 (chroma), scan_mode 0, or 1 / 2 with log2w <= 3; tr_skip the bin value.
// sig_cg: bit (x + y * groups_per_side) set where group (x, y) holds a coefficient; 0 returns 0 (rdo.c:165-173).
template <class Coeffs, class Ctx>
__device__ __forceinline__ u32 coeff_cabac_count(const Coeffs &cf, const Ctx &ctx, u32 range, int log2w, int type, int scan_mode, u32 tr_skip,
                                                 const coeff_cabac_flags f, unsigned long long sig_cg)
{
  if (!sig_cg) return 0;
  coeff_coder<Ctx> cod = { ctx, range, 0u };
  const int lg = log2w - 2, g = 1 << lg;
  const u8 *cgs = lg == 0 ? c_cc_scans.cg2[0] : lg == 1 ? c_cc_scans.cg2[scan_mode] : lg == 2 ? c_cc_scans.cg4 : c_cc_scans.cg8;   // lg 0: entry 0 = (0, 0)
  const u8 *inner = c_cc_scans.inner[scan_mode];
  // the last group and the last coefficient in scan order (:160-172)
  int cg_last = g * g - 1;
  while (!(sig_cg >> ((cgs[cg_last] & 15) + ((cgs[cg_last] >> 4) << lg)) & 1ull)) --cg_last;
  int p_last = 15;
  {
    const int gx = (cgs[cg_last] & 15) << 2, gy = (cgs[cg_last] >> 4) << 2;
    while (p_last > 0 && !cf.at(gx + (inner[p_last] & 15), gy + (inner[p_last] >> 4))) --p_last;
  }
  if (log2w == 2 && f.trskip_enable) cod.bin(type == 0 ? CC_TS_LUMA : CC_TS_CHROMA, tr_skip ? 1u : 0u);
  cod.last_xy(((cgs[cg_last] & 15) << 2) + (inner[p_last] & 15), ((cgs[cg_last] >> 4) << 2) + (inner[p_last] >> 4), log2w, type, scan_mode);

  const int base_sig = type == 0 ? CC_SIG_LUMA : CC_SIG_CHROMA;
  int c1 = 1;
  for (int i = cg_last; i >= 0; --i) {
    const int cg_x = cgs[i] & 15, cg_y = cgs[i] >> 4, gx = cg_x << 2, gy = cg_y << 2;
    const bool last_group = i == cg_last;
    u32 mask = last_group ? 1u << p_last : 0u;                 // bit p: the coefficient at position p of the group's scan is not zero
    const u32 right = (cg_x < g - 1 && (sig_cg >> (cg_x + 1 + (cg_y << lg)) & 1ull)) ? 1u : 0u;
    const u32 lower = (cg_y < g - 1 && (sig_cg >> (cg_x + ((cg_y + 1) << lg)) & 1ull)) ? 1u : 0u;
    bool coded = true;
    if (!last_group && i != 0) {                               // coded_sub_block_flag; inferred for the last group and the first
      coded = (sig_cg >> (cg_x + (cg_y << lg)) & 1ull) != 0;
      cod.bin(CC_SIG_CG + type + (int)(right | lower), coded ? 1u : 0u);   // kvz_context_get_sig_coeff_group, context.c:303-315
    }
    if (coded) {
      const int pattern = (int)(right + (lower << 1));       // kvz_context_calc_pattern_sig_ctx; not looked at for a 4x4 TU
      for (int p = last_group ? p_last - 1 : 15; p >= 0; --p) {
        const int x = gx + (inner[p] & 15), y = gy + (inner[p] >> 4);
        const u32 sig = cf.at(x, y) != 0 ? 1u : 0u;
        if (p > 0 || i == 0 || mask) cod.bin(base_sig + cc_sig_ctx_inc(pattern, scan_mode, x, y, log2w, type), sig);   // else inferred 1
        mask |= sig << p;
      }
    }
    if (!mask) continue;
    const u32 nnz = (u32)__popc(mask);
    const bool hidden = (31 - __clz((int)mask)) - (__ffs((int)mask) - 1) >= 4 && !f.lossless;
    int ctx_set = (i > 0 && type == 0) ? 2 : 0;
    if (c1 == 0) ++ctx_set;
    c1 = 1;
    const int base_one = (type == 0 ? CC_ONE_LUMA : CC_ONE_CHROMA) + 4 * ctx_set;
    int first_c2 = -1;                                         // the value of the first coefficient above 1
    u32 m = mask;
    for (int idx = 0; idx < 8 && m; ++idx) {                   // coeff_abs_level_greater1_flag: the first 8, from the scan's end
      const int p = 31 - __clz((int)m);
      m &= ~(1u << p);
      const int v = cf.at(gx + (inner[p] & 15), gy + (inner[p] >> 4)), a = v < 0 ? -v : v;
      cod.bin(base_one + c1, a > 1 ? 1u : 0u);
      if (a > 1) { c1 = 0; if (first_c2 < 0) first_c2 = a; }
      else if (c1 < 3 && c1 > 0) ++c1;
    }
    if (c1 == 0 && first_c2 >= 0) cod.bin((type == 0 ? CC_ABS_LUMA : CC_ABS_CHROMA) + ctx_set, first_c2 > 2 ? 1u : 0u);
    cod.bits += (f.signhide && hidden) ? nnz - 1 : nnz;      // coeff_sign_flag
    if (c1 == 0 || nnz > 8) {                                  // coeff_abs_level_remaining
      int first_coeff2 = 1;
      u32 rice = 0;
      m = mask;
      for (int idx = 0; m; ++idx) {
        const int p = 31 - __clz((int)m);
        m &= ~(1u << p);
        const int v = cf.at(gx + (inner[p] & 15), gy + (inner[p] >> 4)), a = v < 0 ? -v : v;
        const int base_level = idx < 8 ? 2 + first_coeff2 : 1;
        if (a >= base_level) {
          cod.remain((u32)(a - base_level), rice);
          if (a > (3 << rice)) rice = rice < 4 ? rice + 1 : 4;
        }
        if (a >= 2) first_coeff2 = 0;
      }
    }
  }
  return cod.bits;
}

}  // namespace kvzhip

// rdoq_core.h -- the reference's rate-distortion optimised quantisation of one TU: what kvz_rdoq (rdo.c:548-881) leaves in dest_coeff,
// with kvz_get_ic_rate (:233-278), kvz_get_coded_level (:297-339), get_rate_last / calc_last_bits (:350-395) and kvz_rdoq_sign_hiding
// (:405-539).  Bit depth 8.
//
// The work is cut where the reference's data flow allows it, so that the callers (rdoq.hip) decide what runs across lanes:
//   rdoq_prepare      per coefficient: level_double and err * err * temp (cost_coeff0); says whether max_abs_level > 0
//   rdoq_recursion    ONE lane: everything between the last position found and best_last_idx_p1 -- levels, the c1 / c2 / ctx_set /
//                     Rice recursion, the zeroing of coefficient groups, the last-position search.  base_cost and block_uncoded_cost
//                     are sums of doubles in scan order; nothing of it may be reordered.
//   rdoq_finish       per coefficient: the sign and the clean-up of :866-876
//   rdoq_sign_hide_group   per coefficient group: the body of the loop of kvz_rdoq_sign_hiding, which touches its own group only
// Memory is handed in by rdoq_mem<S>: arrays indexed by the raster position of a coefficient, element i at [i * S], so that a wave
// keeps one TU (S = 1) or every lane its own 4x4 TU, lane-interleaved (S = 64).  Contexts are read and never written: kvz_rdoq
// prices with them and updates none.  A context byte is masked before it indexes the price table and every other index derives
// from the TU's geometry, so no coefficient, context, lambda or table value can cause an access outside an array.
//
// All cost arithmetic is IEEE binary64 in the reference's operation order; the reference's object code holds no fused
// multiply-add, so contraction is off for everything below.  No reciprocal, no fast-math: `/` on doubles is the correctly rounded one.
#pragma once
#include "coeff_cabac_core.h"

#pragma clang fp contract(off)

namespace kvzhip {

typedef long long i64;

enum : int { RQ_FRAC_BITS = 15, RQ_ONE_BIT = 1 << 15, RQ_C1FLAG_NUMBER = 8, RQ_C2FLAG_NUMBER = 1, RQ_SBH_THRESHOLD = 4 };   // rdo.h:65-66, encoderstate.h:355-356
#define RQ_MAX_DOUBLE 1.7e+308                                   // global.h:269

// the state's nine context bytes beyond kvz_hip_coeff_ctx, in the order of kvz_hip_rdoq_state from root_cbf on
enum : int { RQ_ROOT_CBF = 0, RQ_CBF_LUMA = 1, RQ_CBF_CHROMA = 5, RQ_STATE_CTX = 9 };

struct rdoq_tu {
  int log2w, type, scan_mode, intra, tr_depth, qp_scaled, q_bits, signhide;
  double lambda;
};

template <int S>
struct rdoq_mem {
  double *c0, *cc, *cs;           // cost_coeff0, cost_coeff, cost_sig
  double *cg_sig;                 // cost_coeffgroup_sig, by the group's scan index
  i32 *ld;                        // level_double
  i32 *sig_inc, *inc, *dec, *qd;  // sh_rates_t (rdo.h:47-60): sig_coeff_inc, inc, dec, quant_delta
  i32 *last_x, *last_y;           // calc_last_bits: up to 10 entries each
  i16 *dst;                       // dest_coeff
  const i16 *coef;
  static constexpr int stride = S;
};

// the context bytes: c = kvz_hip_coeff_ctx.ctx, s = the nine bytes of kvz_hip_rdoq_state
struct rdoq_ctx {
  const u8 *c, *s;
  __device__ __forceinline__ u32 bits(int i, u32 bin) const { return c_entropy_bits[(c[i] ^ bin) & 127u]; }      // CTX_ENTROPY_BITS
  __device__ __forceinline__ u32 state_bits(int i, u32 bin) const { return c_entropy_bits[(s[i] ^ bin) & 127u]; }
};

// where the scan goes: group k of the TU's group scan, position p of the 4x4 scan -> raster index
struct rdoq_scan {
  const u8 *cgs, *inner;
  int log2w;
  __device__ __forceinline__ int cg_x(int k) const { return cgs[k] & 15; }
  __device__ __forceinline__ int cg_y(int k) const { return cgs[k] >> 4; }
  __device__ __forceinline__ int x(int s) const { return ((cgs[s >> 4] & 15) << 2) + (inner[s & 15] & 15); }
  __device__ __forceinline__ int y(int s) const { return ((cgs[s >> 4] >> 4) << 2) + (inner[s & 15] >> 4); }
  __device__ __forceinline__ int blk(int s) const { return (y(s) << log2w) + x(s); }
};
__device__ __forceinline__ rdoq_scan rdoq_make_scan(int log2w, int scan_mode)
{
  const int lg = log2w - 2;
  return { lg == 0 ? c_cc_scans.cg2[0] : lg == 1 ? c_cc_scans.cg2[scan_mode] : lg == 2 ? c_cc_scans.cg4 : c_cc_scans.cg8, c_cc_scans.inner[scan_mode], log2w };
}

// rdo.c:627-630 / :666-673: level_double and the cost of coding nothing; returns max_abs_level
template <class M>
__device__ __forceinline__ u32 rdoq_prepare(const M &m, int blk, i32 q, double temp, int q_bits)
{
  const i32 c = m.coef[blk * M::stride];
  const i64 prod = (i64)(c < 0 ? -c : c) * q, cap = 0x7fffffffll - (1ll << (q_bits - 1));
  const i32 level_double = (i32)(prod < cap ? prod : cap);
  m.ld[blk * M::stride] = level_double;
  const double err = (double)level_double;
  m.c0[blk * M::stride] = err * err * temp;
  return (u32)(level_double + (1 << (q_bits - 1))) >> q_bits;
}

// kvz_get_ic_rate, rdo.c:233-278; one_i / abs_i are indices into kvz_hip_coeff_ctx.ctx
__device__ __forceinline__ i32 rdoq_ic_rate(const rdoq_ctx &ctx, u32 abs_level, int one_i, int abs_i, u32 rice, u32 c1_idx, u32 c2_idx)
{
  i32 rate = RQ_ONE_BIT;
  const u32 base_level = c1_idx < RQ_C1FLAG_NUMBER ? 2u + (c2_idx < RQ_C2FLAG_NUMBER ? 1u : 0u) : 1u;
  if (abs_level >= base_level) {
    i32 symbol = (i32)(abs_level - base_level), length;
    if (symbol < (i32)(3u << rice)) {
      length = symbol >> rice;
      rate += (length + 1 + (i32)rice) * RQ_ONE_BIT;
    } else {
      length = (i32)rice;
      symbol -= (i32)(3u << rice);
      while (symbol >= (1 << length)) { symbol -= 1 << length; ++length; }
      rate += (3 + length + 1 - (i32)rice + length) * RQ_ONE_BIT;
    }
    if (c1_idx < RQ_C1FLAG_NUMBER) {
      rate += (i32)ctx.bits(one_i, 1);
      if (c2_idx < RQ_C2FLAG_NUMBER) rate += (i32)ctx.bits(abs_i, 1);
    }
  } else if (abs_level == 1) {
    rate += (i32)ctx.bits(one_i, 0);
  } else if (abs_level == 2) {
    rate += (i32)ctx.bits(one_i, 1);
    rate += (i32)ctx.bits(abs_i, 0);
  }
  return rate;
}

// kvz_get_coded_level, rdo.c:297-339.  coded_cost0 is read where the reference reads it; sig_i indexes kvz_hip_coeff_ctx.ctx.
__device__ __forceinline__ u32 rdoq_coded_level(const rdoq_ctx &ctx, double lambda, double &coded_cost, double coded_cost0, double &coded_cost_sig,
                                                i32 level_double, u32 max_abs_level, int sig_i, int one_i, int abs_i, u32 rice, u32 c1_idx, u32 c2_idx,
                                                int q_bits, double temp, bool last)
{
  double cur_cost_sig = 0;
  u32 best_abs_level = 0;
  if (!last && max_abs_level < 3) {
    coded_cost_sig = lambda * ctx.bits(sig_i, 0);
    coded_cost = coded_cost0 + coded_cost_sig;
    if (max_abs_level == 0) return best_abs_level;
  } else {
    coded_cost = RQ_MAX_DOUBLE;
  }
  if (!last) cur_cost_sig = lambda * ctx.bits(sig_i, 1);
  const i32 min_abs_level = max_abs_level > 1 ? (i32)max_abs_level - 1 : 1;
  for (i32 abs_level = (i32)max_abs_level; abs_level >= min_abs_level; --abs_level) {
    const double err = (double)(level_double - abs_level * (1 << q_bits));
    double cur_cost = err * err * temp + lambda * rdoq_ic_rate(ctx, (u32)abs_level, one_i, abs_i, rice, c1_idx, c2_idx);
    cur_cost += cur_cost_sig;
    if (cur_cost < coded_cost) {
      best_abs_level = (u32)abs_level;
      coded_cost = cur_cost;
      coded_cost_sig = cur_cost_sig;
    }
  }
  return best_abs_level;
}

// rdo.c:648-864 for a TU whose last position with max_abs_level > 0 is last_scanpos >= 0; ld and c0 hold rdoq_prepare's values for
// every position up to it.  Returns best_last_idx_p1.  dst holds the unsigned levels of the positions up to last_scanpos afterwards.
template <class M>
__device__ __forceinline__ int rdoq_recursion(const M &m, const rdoq_ctx &ctx, const rdoq_scan &sc, const rdoq_tu &t, const double *err_scale, int last_scanpos)
{
  constexpr int S = M::stride;
  const int log2w = t.log2w, type = t.type, lg = log2w - 2, g = 1 << lg, q_bits = t.q_bits;
  const double lambda = t.lambda;
  const int base_sig = type == 0 ? CC_SIG_LUMA : CC_SIG_CHROMA, base_one = type == 0 ? CC_ONE_LUMA : CC_ONE_CHROMA,
            base_abs = type == 0 ? CC_ABS_LUMA : CC_ABS_CHROMA;
  const int cg_last_scanpos = last_scanpos >> 4;
  unsigned long long sig_cg = 0;                                   // sig_coeffgroup_flag, bit x + y * g
  double block_uncoded_cost = 0, base_cost = 0;
  u32 ctx_set = (last_scanpos > 0 && type == 0) ? 2 : 0, rice = 0, c1_idx = 0, c2_idx = 0;
  int c1 = 1, c2 = 0;

  for (int k = cg_last_scanpos; k >= 0; --k) m.cg_sig[k * S] = 0;

  {                                                                 // calc_last_bits, rdo.c:366-395
    const int ctx_offset = type ? 0 : lg * 3 + ((lg + 1) >> 2), shift = type ? lg : (lg + 3) >> 2, top = c_cc_group_idx[(1 << log2w) - 1];
    const int bx = (type ? CC_LAST_X_CHROMA : CC_LAST_X_LUMA) + ctx_offset, by = (type ? CC_LAST_Y_CHROMA : CC_LAST_Y_LUMA) + ctx_offset;
    i32 bits_x = 0, bits_y = 0;
    for (int k = 0; k < top; ++k) {
      m.last_x[k * S] = bits_x + (i32)ctx.bits(bx + (k >> shift), 0);
      bits_x += (i32)ctx.bits(bx + (k >> shift), 1);
      m.last_y[k * S] = bits_y + (i32)ctx.bits(by + (k >> shift), 0);
      bits_y += (i32)ctx.bits(by + (k >> shift), 1);
    }
    m.last_x[top * S] = bits_x;
    m.last_y[top * S] = bits_y;
  }

  for (int cg = cg_last_scanpos; cg >= 0; --cg) {
    const int cg_x = sc.cg_x(cg), cg_y = sc.cg_y(cg), cg_bit = cg_x + (cg_y << lg);
    const u32 right = (cg_x < g - 1 && (sig_cg >> (cg_bit + 1) & 1ull)) ? 1u : 0u;
    const u32 lower = (cg_y < g - 1 && (sig_cg >> (cg_bit + g) & 1ull)) ? 1u : 0u;
    const int pattern = (int)(right + (lower << 1));              // kvz_context_calc_pattern_sig_ctx; not looked at for a 4x4 TU
    double coded_level_and_dist = 0, uncoded_dist = 0, sig_cost = 0, sig_cost_0 = 0;   // rd_stats
    int nnz_before_pos0 = 0;
    for (int p = 15; p >= 0; --p) {
      const int scanpos = cg * 16 + p;
      if (scanpos > last_scanpos) continue;
      const int x = sc.x(scanpos), y = sc.y(scanpos), blk = (y << log2w) + x;
      const double temp = err_scale[blk];
      const i32 level_double = m.ld[blk * S];
      const u32 max_abs_level = (u32)(level_double + (1 << (q_bits - 1))) >> q_bits;
      const double cost0 = m.c0[blk * S];
      block_uncoded_cost += cost0;
      const int one_i = base_one + (int)(4 * ctx_set) + c1, abs_i = base_abs + (int)ctx_set + c2;
      double cost_coeff, cost_sig = 0;
      u32 level;
      if (scanpos == last_scanpos) {
        level = rdoq_coded_level(ctx, lambda, cost_coeff, cost0, cost_sig, level_double, max_abs_level, 0, one_i, abs_i, rice, c1_idx, c2_idx, q_bits, temp, true);
        // max_abs_level > 0 here, so the loop of kvz_get_coded_level runs and leaves cost_sig = cur_cost_sig = 0
      } else {
        const int sig_i = base_sig + cc_sig_ctx_inc(pattern, t.scan_mode, x, y, log2w, type);
        level = rdoq_coded_level(ctx, lambda, cost_coeff, cost0, cost_sig, level_double, max_abs_level, sig_i, one_i, abs_i, rice, c1_idx, c2_idx, q_bits, temp, false);
        if (t.signhide) m.sig_inc[blk * S] = (i32)ctx.bits(sig_i, 1) - (i32)ctx.bits(sig_i, 0);
      }
      if (t.signhide) {
        if (scanpos == last_scanpos) m.sig_inc[blk * S] = 0;      // rdo.c:636
        m.qd[blk * S] = (level_double - (i32)level * (1 << q_bits)) >> (q_bits - 8);
        if (level > 0) {
          const i32 rate_now = rdoq_ic_rate(ctx, level, one_i, abs_i, rice, c1_idx, c2_idx);
          m.inc[blk * S] = rdoq_ic_rate(ctx, level + 1, one_i, abs_i, rice, c1_idx, c2_idx) - rate_now;
          m.dec[blk * S] = rdoq_ic_rate(ctx, level - 1, one_i, abs_i, rice, c1_idx, c2_idx) - rate_now;
        } else {
          m.inc[blk * S] = (i32)ctx.bits(one_i, 0);
        }
      }
      const i16 stored = (i16)level;                                // (coeff_t)level: what the reference reads back below
      m.dst[blk * S] = stored;
      m.cc[blk * S] = cost_coeff;
      m.cs[blk * S] = cost_sig;
      base_cost += cost_coeff;

      const u32 base_level = c1_idx < RQ_C1FLAG_NUMBER ? 2u + (c2_idx < RQ_C2FLAG_NUMBER ? 1u : 0u) : 1u;
      if (level >= base_level && level > (3u << rice)) rice = rice < 4 ? rice + 1 : 4;
      if (level >= 1) ++c1_idx;
      if (level > 1) {
        c1 = 0;
        c2 += c2 < 2;
        ++c2_idx;
      } else if (c1 < 3 && c1 > 0 && level) {
        ++c1;
      }
      if (p == 0 && scanpos > 0) {                                  // context set update, rdo.c:732-743
        c2 = 0;
        rice = 0;
        c1_idx = 0;
        c2_idx = 0;
        ctx_set = (scanpos == 16 || type != 0) ? 0 : 2;
        if (c1 == 0) ++ctx_set;
        c1 = 1;
      }
      sig_cost += cost_sig;
      if (p == 0) sig_cost_0 = cost_sig;
      if (stored) {
        sig_cg |= 1ull << cg_bit;
        coded_level_and_dist += cost_coeff - cost_sig;
        uncoded_dist += cost0;
        if (p != 0) ++nnz_before_pos0;
      }
    }

    if (cg) {                                                       // rdo.c:759-812
      const int cg_ctx = CC_SIG_CG + type + (int)(right | lower);  // kvz_context_get_sig_coeff_group
      if (!(sig_cg >> cg_bit & 1ull)) {
        const double c = lambda * ctx.bits(cg_ctx, 0);
        m.cg_sig[cg * S] = c;
        base_cost += c - sig_cost;
      } else if (cg < cg_last_scanpos) {
        if (nnz_before_pos0 == 0) {
          base_cost -= sig_cost_0;
          sig_cost -= sig_cost_0;
        }
        double cost_zero_cg = base_cost;
        const double c1g = lambda * ctx.bits(cg_ctx, 1);
        m.cg_sig[cg * S] = c1g;
        base_cost += c1g;
        cost_zero_cg += lambda * ctx.bits(cg_ctx, 0);
        cost_zero_cg += uncoded_dist;
        cost_zero_cg -= coded_level_and_dist;
        cost_zero_cg -= sig_cost;
        if (cost_zero_cg < base_cost) {
          sig_cg &= ~(1ull << cg_bit);
          base_cost = cost_zero_cg;
          m.cg_sig[cg * S] = lambda * ctx.bits(cg_ctx, 0);
          for (int p = 15; p >= 0; --p) {
            const int blk = sc.blk(cg * 16 + p);
            if (m.dst[blk * S]) {
              m.dst[blk * S] = 0;
              m.cc[blk * S] = m.c0[blk * S];
              m.cs[blk * S] = 0;
            }
          }
        }
      }
    } else {
      sig_cg |= 1ull << cg_bit;
    }
  }

  // ===== the last position, rdo.c:815-864
  double best_cost;
  int best_last_idx_p1 = 0;
  if (!t.intra && !type) {
    best_cost = block_uncoded_cost + lambda * ctx.state_bits(RQ_ROOT_CBF, 0);
    base_cost += lambda * ctx.state_bits(RQ_ROOT_CBF, 1);
  } else {
    const int cbf_i = type ? RQ_CBF_CHROMA + t.tr_depth : RQ_CBF_LUMA + (t.tr_depth ? 0 : 1);
    best_cost = block_uncoded_cost + lambda * ctx.state_bits(cbf_i, 0);
    base_cost += lambda * ctx.state_bits(cbf_i, 1);
  }
  bool found_last = false;
  for (int cg = cg_last_scanpos; cg >= 0 && !found_last; --cg) {
    const int cg_bit = sc.cg_x(cg) + (sc.cg_y(cg) << lg);
    base_cost -= m.cg_sig[cg * S];
    if (!(sig_cg >> cg_bit & 1ull)) continue;
    for (int p = 15; p >= 0; --p) {
      const int scanpos = cg * 16 + p;
      if (scanpos > last_scanpos) continue;
      const int x = sc.x(scanpos), y = sc.y(scanpos), blk = (y << log2w) + x;
      const i16 d = m.dst[blk * S];
      if (d) {
        const int px = t.scan_mode == 2 ? y : x, py = t.scan_mode == 2 ? x : y;   // get_rate_last, rdo.c:350-364, :845
        const u32 ctx_x = c_cc_group_idx[px], ctx_y = c_cc_group_idx[py];
        double cost = (double)(m.last_x[ctx_x * S] + m.last_y[ctx_y * S]);
        if (ctx_x > 3) cost += (double)((u32)RQ_ONE_BIT * ((ctx_x - 2) >> 1));
        if (ctx_y > 3) cost += (double)((u32)RQ_ONE_BIT * ((ctx_y - 2) >> 1));
        const double cost_last = lambda * cost;
        const double total = base_cost + cost_last - m.cs[blk * S];
        if (total < best_cost) {
          best_last_idx_p1 = scanpos + 1;
          best_cost = total;
        }
        if (d > 1) { found_last = true; break; }
        base_cost -= m.cc[blk * S];
        base_cost += m.c0[blk * S];
      } else {
        base_cost -= m.cs[blk * S];
      }
    }
  }
  return best_last_idx_p1;
}

// rdo.c:866-876 for scan position s of the whole TU (positions behind last_scanpos come out 0 as well, rdo.c:639); returns the level
// that the position adds to abs_sum
template <class M>
__device__ __forceinline__ u32 rdoq_finish(const M &m, int blk, int s, int best_last_idx_p1)
{
  constexpr int S = M::stride;
  if (s >= best_last_idx_p1) { m.dst[blk * S] = 0; return 0; }
  const i32 level = m.dst[blk * S];
  m.dst[blk * S] = (i16)(m.coef[blk * S] < 0 ? -level : level);
  return (u32)level;
}

// rd_factor of kvz_rdoq_sign_hiding, rdo.c:416-421, at bit depth 8: two correctly rounded divisions
__device__ __forceinline__ i64 rdoq_rd_factor(int qp_scaled, double lambda)
{
  const int inv_quant_scales[6] = { 40, 45, 51, 57, 64, 72 };     // kvz_g_inv_quant_scales, scalinglist.c:67
  const int inv_quant = inv_quant_scales[qp_scaled % 6];
  return (i64)(inv_quant * inv_quant * (1 << (2 * (qp_scaled / 6))) / lambda / 16 / 1 + 0.5);
}

// the body of the loop of kvz_rdoq_sign_hiding for group cg_scan <= last_cg, rdo.c:424-538
template <class M>
__device__ __forceinline__ void rdoq_sign_hide_group(const M &m, const rdoq_scan &sc, int cg_scan, int last_cg, i64 rd_factor)
{
  constexpr int S = M::stride;
  const i64 max_i64 = 0x7fffffffffffffffll;
  const int at = cg_scan << 4;
  int last_nz = -1, first_nz = 16;
  for (int p = 15; p >= 0; --p) if (m.dst[sc.blk(at + p) * S]) { last_nz = p; break; }
  for (int p = 0; p <= last_nz; ++p) if (m.dst[sc.blk(at + p) * S]) { first_nz = p; break; }
  if (last_nz - first_nz < RQ_SBH_THRESHOLD) return;
  const i32 signbit = m.dst[sc.blk(at + first_nz) * S] <= 0;
  u32 abs_coeff_sum = 0;
  for (int p = first_nz; p <= last_nz; ++p) abs_coeff_sum += (u32)(i32)m.dst[sc.blk(at + p) * S];
  if ((u32)signbit == (abs_coeff_sum & 1u)) return;

  i64 best_cost = max_i64;
  int best_pos = 0, best_change = 0;
  for (int p = cg_scan == last_cg ? last_nz : 15; p >= 0; --p) {
    const int pos = sc.blk(at + p);
    const i64 quant_cost_in_bits = rd_factor * m.qd[pos * S];
    const i32 v = m.dst[pos * S], abs_coeff = v < 0 ? -v : v;
    i64 cost;
    int change;
    if (abs_coeff != 0) {
      i64 inc_bits = m.inc[pos * S], dec_bits = m.dec[pos * S];
      if (abs_coeff == 1) dec_bits -= RQ_ONE_BIT + m.sig_inc[pos * S];
      if (cg_scan == last_cg && last_nz == p && abs_coeff == 1) dec_bits -= 4 * RQ_ONE_BIT;
      inc_bits = -quant_cost_in_bits + inc_bits * (1 << (15 - RQ_FRAC_BITS));
      dec_bits = quant_cost_in_bits + dec_bits * (1 << (15 - RQ_FRAC_BITS));
      if (inc_bits < dec_bits) {
        change = 1;
        cost = inc_bits;
      } else {
        change = -1;
        cost = dec_bits;
        if (p == first_nz && abs_coeff == 1) cost = max_i64;
      }
    } else {
      const i32 bits = RQ_ONE_BIT + m.inc[pos * S] + m.sig_inc[pos * S];
      cost = -(quant_cost_in_bits < 0 ? -quant_cost_in_bits : quant_cost_in_bits) + (i64)(bits * (1 << (15 - RQ_FRAC_BITS)));
      change = 1;
      if (p < first_nz && ((m.coef[pos * S] >= 0) ? 0 : 1) != signbit) cost = max_i64;
    }
    if (cost < best_cost) { best_cost = cost; best_pos = pos; best_change = change; }
  }
  const i16 b = m.dst[best_pos * S];
  if (b == 32767 || b == -32768) best_change = -1;
  m.dst[best_pos * S] = (i16)(m.coef[best_pos * S] >= 0 ? b + best_change : b - best_change);
}

}  // namespace kvzhip

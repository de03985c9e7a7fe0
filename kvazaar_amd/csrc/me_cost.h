// me_cost.h -- the MV cost model of the motion search (me_search_core.h): bits of a vector against the two MV predictors
// and the merge list, from the exp-Golomb lengths or, with --mv-rdo, from the CABAC model; and fracmv_within_tile.
#pragma once
#include "kvz_hip_internal.h"
#include "cabac_tables.h"

namespace kvzhip {

// calc_mvd_cost / fracmv_within_tile on the flattened encoder state (include/kvz_hip.h).  The descriptor is copied
// into (scalar) registers once per PU: the cost model runs for every one of the ~60 candidates of a search, and
// reading the merge list from memory each time made scalar loads the longest chain of the kernel.
// --mv-rdo: the CABAC probability tables are those of cabac_tables.h
// what kvz_calc_mvd_cost_cabac reads of state->cabac, and the bits its counting-mode encoder produces: the count
// (23 - bits_left) + 8 * num_buffered_bytes (cabac.c:95-140) is the number of renormalisation shifts, a function of `range`
// and the context states alone
struct cabac_model {
  u32 range;
  u32 ctx[7];        // uc_state of merge_flag, merge_idx, ref_pic[0], ref_pic[1], mvd[0], mvd[1], mvp_idx[0]
  template <int C>
  __device__ __forceinline__ u32 bin(bool b)           // kvz_cabac_encode_bin, cabac.c:90-122
  {
    const u32 uc = ctx[C], st = uc >> 1, lps = c_range_lps[st * 4 + ((range >> 6) & 3)];
    range -= lps;
    if ((b ? 1u : 0u) != (uc & 1u)) {
      const u32 n = (u32)__clz((int)(lps >> 3)) - 26u;
      range = lps << n;
      ctx[C] = ((u32)c_trans_lps[st] << 1) | ((uc & 1u) ^ (st == 0 ? 1u : 0u));
      return n;
    }
    ctx[C] = ((st < 62 ? st + 1 : st) << 1) | (uc & 1u);
    if (range >= 256) return 0;
    range <<= 1;
    return 1;
  }
  // kvz_cabac_write_ep_ex_golomb(symbol, 1), cabac.c:535-570: number of bypass bins
  static __device__ __forceinline__ u32 ex_golomb1(u32 symbol)
  {
    u32 n = 0, count = 1;
    while (symbol >= (1u << count)) { ++n; symbol -= 1u << count; ++count; }
    return n + 1 + count;
  }
  // kvz_encode_mvd, encode_coding_tree.c:1156-1202
  __device__ __forceinline__ u32 mvd(int hor, int ver)
  {
    const u32 ah = (u32)(hor < 0 ? -hor : hor), av = (u32)(ver < 0 ? -ver : ver);
    u32 bits = bin<4>(hor != 0);
    bits += bin<4>(ver != 0);
    if (hor) bits += bin<5>(ah > 1);
    if (ver) bits += bin<5>(av > 1);
    if (hor) bits += (ah > 1 ? ex_golomb1(ah - 2) : 0u) + 1u;
    if (ver) bits += (av > 1 ? ex_golomb1(av - 2) : 0u) + 1u;
    return bits;
  }
};

// RDO: --mv-rdo cost model.  CONSTR: some fracmv_within_tile rule is active (WPP / OWF availability or an mv_constraint); the
// common unconstrained search is compiled without the rule and its scalar state (the kernels sit at the edge of their SGPR budget).
template <bool RDO, bool CONSTR = true>
struct me_cost_model_t {
  int px, py, pw, ph;
  int cand[2][2];
  int n_merge;
  int mx[5], my[5];
  u32 usable, same_ref;                                // bit i = merge[i].usable / .same_ref
  u32 mkey[5];                                         // merge vector i as (x & 0xffff) | y << 16, for merge_match
  int lambda_cost, wpp_owf, ref_delay_px, max_down, max_right;
  int constraint, ox, oy, tw, th;                      // cfg.mv_constraint, tile-relative origin of the PU, tile size
  cabac_model cab;                                     // RDO only
  int rdo_ref_idx, rdo_refs_before;

  __device__ __forceinline__ me_cost_model_t(const kvz_hip_me_pu &pu, const kvz_hip_me_params &prm)
  {
    if (RDO) {
      const kvz_hip_me_cabac &c = prm.cabac[pu.reserved];
      cab.range = c.range;
#pragma unroll
      for (int i = 0; i < 7; ++i) cab.ctx[i] = c.ctx[i];
      rdo_ref_idx = prm.ref_idx; rdo_refs_before = prm.refs_before;
    }
    px = pu.x; py = pu.y; pw = pu.width; ph = pu.height;
    cand[0][0] = pu.mv_cand[0][0]; cand[0][1] = pu.mv_cand[0][1]; cand[1][0] = pu.mv_cand[1][0]; cand[1][1] = pu.mv_cand[1][1];
    n_merge = pu.num_merge_cand;
    usable = 0; same_ref = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      mx[i] = pu.merge[i].mv[0]; my[i] = pu.merge[i].mv[1];
      mkey[i] = ((u32)mx[i] & 0xffffu) | ((u32)my[i] << 16);
      if (i < n_merge && pu.merge[i].usable) usable |= 1u << i;
      if (pu.merge[i].same_ref) same_ref |= 1u << i;
    }
    lambda_cost = prm.lambda_cost; wpp_owf = prm.wpp_owf; ref_delay_px = prm.ref_delay_px;
    max_down = prm.max_ref_lcu_down; max_right = prm.max_ref_lcu_right;
    constraint = prm.mv_constraint;
    ox = pu.x - prm.tile_x; oy = pu.y - prm.tile_y; tw = prm.tile_w; th = prm.tile_h;
  }

  // fracmv_within_tile (search_inter.c:87-176), all mv_constraint branches; quarter-pel vector.  info->origin is
  // relative to the tile, and so are the LCU indices of the availability rule (C division: truncation toward zero).
  __device__ __forceinline__ bool within(int x, int y) const
  {
    if (!CONSTR) return true;
    const bool frac_luma = x % 4 != 0 || y % 4 != 0, frac_chroma = x % 8 != 0 || y % 8 != 0;
    if (wpp_owf) {
      int margin = frac_luma ? 4 : (frac_chroma ? 2 : 0);
      margin += ref_delay_px;
      const int lcu_x = ox / 64, lcu_y = oy / 64;
      const int mv_lcu_x = ((ox + pw + margin) * 4 + x) / (64 << 2) - lcu_x;
      const int mv_lcu_y = ((oy + ph + margin) * 4 + y) / (64 << 2) - lcu_y;
      if (mv_lcu_y > max_down) return false;
      if (mv_lcu_x + mv_lcu_y > max_down + max_right) return false;
    }
    if (constraint == 0) return true;
    const int margin = constraint == 4 ? (frac_luma ? 4 << 2 : (frac_chroma ? 2 << 2 : 0)) : 0;
    const int ax = ox * 4 + x, ay = oy * 4 + y;
    const int from_right = (tw << 2) - (ax + (pw << 2)), from_bottom = (th << 2) - (ay + (ph << 2));
    return ax >= margin && ay >= margin && from_right >= margin && from_bottom >= margin;
  }
  // get_ep_ex_golomb_bitcost (:235-254)
  static __device__ __forceinline__ u32 golomb(u32 symbol)
  {
    symbol += 2;
    // the reference's four range tests add up to 2 * floor(log2(symbol)) while symbol < 2^16 (they test bits 8, 4, 2, 1
    // of the exponent once each); vectors are int16, so only a difference of two extreme vectors gets past that
    if (__builtin_expect(symbol < (1u << 16), 1)) return 2u * (31u - (u32)__builtin_clz(symbol));
    u32 bins = 0;
    if (symbol >= 1u << 8) { bins += 16; symbol >>= 8; }
    if (symbol >= 1u << 4) { bins += 8; symbol >>= 4; }
    if (symbol >= 1u << 2) { bins += 4; symbol >>= 2; }
    if (symbol >= 1u << 1) { bins += 2; }
    return bins;
  }
  // get_mvd_coding_cost (:310-323): whole bits, the fixed-point rounding is exact
  static __device__ __forceinline__ u32 mvd_bits(int dx, int dy)
  {
    return golomb((u32)(dx < 0 ? -dx : dx)) + golomb((u32)(dy < 0 ? -dy : dy));
  }
  // select_mv_cand (:326-370).  |d| + 2 of each vector component is one v_sad_u32 on operands moved into the unsigned
  // range, the exp-Golomb length of a component 2 * (31 - clz(|d| + 2)) (see golomb), so a candidate costs
  // 124 - 2 * (clz + clz) bits and the cheaper of the two is the one with the larger clz sum.
  __device__ __forceinline__ int select_cand(int mvx, int mvy, u32 &cost) const
  {
    constexpr u32 BIAS = 1u << 20;                       // |mv|, |candidate| < 2^18: sums stay positive
    const u32 xb = (u32)mvx + BIAS, yb = (u32)mvy + BIAS;
    u32 s[4];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const u32 cx = (u32)cand[c][0] + BIAS, cy = (u32)cand[c][1] + BIAS;
      s[2 * c] = (xb > cx ? xb - cx : cx - xb) + 2u;     // v_sad_u32
      s[2 * c + 1] = (yb > cy ? yb - cy : cy - yb) + 2u;
    }
    if (__builtin_expect(((s[0] | s[1] | s[2] | s[3]) >> 16) != 0, 0)) {        // a difference of two extreme vectors
      const u32 c1 = mvd_bits(mvx - cand[0][0], mvy - cand[0][1]), c2 = mvd_bits(mvx - cand[1][0], mvy - cand[1][1]);
      cost = c1 < c2 ? c1 : c2;
      return c2 < c1 ? 1 : 0;
    }
    const u32 z1 = (u32)__builtin_clz(s[0]) + (u32)__builtin_clz(s[1]), z2 = (u32)__builtin_clz(s[2]) + (u32)__builtin_clz(s[3]);
    cost = 124u - 2u * (z1 > z2 ? z1 : z2);
    return z2 > z1 ? 1 : 0;
  }
  // index of the first merge candidate that codes (x, y) (quarter-pel) for this reference, or -1
  __device__ __forceinline__ int merge_match(int x, int y) const
  {
    // one compare per candidate on the packed vector; a vector outside int16 matches nothing (the candidates are int16)
    const u32 key = ((u32)x & 0xffffu) | ((u32)y << 16), live = usable & same_ref;
    int m = -1;
#pragma unroll
    for (int i = 4; i >= 0; --i)
      if ((live >> i & 1u) && mkey[i] == key) m = i;
    return ((u32)(x + 32768) < 65536u && (u32)(y + 32768) < 65536u) ? m : -1;
  }
  // kvz_get_mvd_coding_cost_cabac (rdo.c:883-903): a fresh copy of the state per call
  __device__ __forceinline__ u32 mvd_bits_cabac(int dx, int dy) const
  {
    cabac_model m = cab;
    return m.mvd(dx, dy);
  }
  // select_mv_cand (:326-370) with --mv-rdo, cost_out == NULL
  __device__ __forceinline__ int select_cand_cabac(int mvx, int mvy) const
  {
    const u32 c1 = mvd_bits_cabac(mvx - cand[0][0], mvy - cand[0][1]), c2 = mvd_bits_cabac(mvx - cand[1][0], mvy - cand[1][1]);
    return c2 < c1 ? 1 : 0;
  }
  // kvz_calc_mvd_cost_cabac (rdo.c:908-1060)
  __device__ __forceinline__ u32 cost_cabac(int x, int y, u32 &bits) const
  {
    const int mi = merge_match(x, y);
    int cur_cand = 0, dx = 0, dy = 0;
    if (mi < 0) {
      const int d1x = x - cand[0][0], d1y = y - cand[0][1], d2x = x - cand[1][0], d2y = y - cand[1][1];
      const u32 c1 = mvd_bits_cabac(d1x, d1y), c2 = mvd_bits_cabac(d2x, d2y);
      if (c2 < c1) { cur_cand = 1; dx = d2x; dy = d2y; } else { dx = d1x; dy = d1y; }
    }
    cabac_model m = cab;
    u32 b = m.template bin<0>(mi >= 0);
    if (mi >= 0) {
      for (int ui = 0; ui < 4; ++ui) {                   // MRG_MAX_NUM_CANDS - 1
        const bool symbol = ui != mi;
        b += ui == 0 ? m.template bin<1>(symbol) : 1u;
        if (!symbol) break;
      }
    } else {
      if (rdo_refs_before > 1) {
        int ref_frame = rdo_ref_idx;
        b += m.template bin<2>(ref_frame != 0);
        if (ref_frame > 0) {
          const int ref_num = rdo_refs_before - 2;
          --ref_frame;
          for (int i = 0; i < ref_num; ++i) {
            const bool symbol = i != ref_frame;
            b += i == 0 ? m.template bin<3>(symbol) : 1u;
            if (!symbol) break;
          }
        }
      }
      b += m.mvd(dx, dy);
      b += m.template bin<6>(cur_cand != 0);
    }
    bits = b;
    return __umul24(b, (u32)lambda_cost);
  }
  // calc_mvd_cost (:373-412)
  __device__ __forceinline__ u32 cost(int x, int y, int mv_shift, u32 &bits) const
  {
    x *= 1 << mv_shift;
    y *= 1 << mv_shift;
    if (RDO) return cost_cabac(x, y, bits);
    const int m = merge_match(x, y);
    if (m >= 0) bits = (u32)m;
    else select_cand(x, y, bits);
    return __umul24(bits, (u32)lambda_cost);            // bits < 2^7, lambda_cost <= 2^20 (checked by the entry): a full-rate multiply
  }
  // mv_in_merge (:260-273), integer-pel vector
  __device__ __forceinline__ bool in_merge(int x, int y) const
  {
    bool hit = false;
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if ((usable >> i & 1u) && ((mx[i] + 2) >> 2) == x && ((my[i] + 2) >> 2) == y) hit = true;
    return hit;
  }
};

}  // namespace kvzhip

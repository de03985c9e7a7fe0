// quant_core.h -- the quantisation arithmetic shared by quant.hip (batched entries), inter_residual.hip and intra_recon_core.h
// (whole-picture entries): the flattened encoder state and the one function that derives it for flat lists, on the host and on the
// device (flat_consts), the one that layers scaling lists over it (sl_consts), quant / dequant of one coefficient and the
// sign-bit-hiding pass.
// Reference: src/strategies/generic/quant-generic.c (cited per function), transform.c:129-143 for the scaled QP.
#pragma once

#include "kvz_hip_internal.h"
#include "transform_core.h"

using namespace kvzhip;

struct quant_consts {
  int q_bits, add, flat_qc, signhide;       // quant
  const int32_t *qtable;                     // per-coefficient factors or nullptr (flat)
  int dq_mode;                               // 0 flat, 1 scaling list (shift > qp/6), 2 scaling list (clip + shl)
  int dq_shift, dq_add, dq_scale;            // mode 0: (q*scale + add) >> shift; mode 1: shift/add; mode 2: shl = dq_shift
  const int32_t *dqtable;
};

// transform.c:129-143; type 0 is luma, every other type chroma
__host__ __device__ inline int scaled_qp(int type, int qp)
{
  const unsigned char chroma_scale[58] = {
     0, 1, 2, 3, 4, 5, 6, 7, 8, 9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,29,30,31,32,
    33,33,34,34,35,35,36,36,37,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51 };
  if (type == 0) return qp;
  int q = qp < 0 ? 0 : (qp > 57 ? 57 : qp);      // CLIP(-qp_offset, 57, qp) with qp_offset 0
  return chroma_scale[q];
}
static int log2i(int w) { int l = 0; while ((1 << l) < w) ++l; return l; }

// The constants of flat lists (no scaling list) for one QP, transform size and colour, quant-generic.c:40-50 and :283-320: the
// ONE place they are derived.  The host calls it per launch (make_consts below), the per-LCU-QP kernels call it per TU or per LCU
// with the QP they read on the device.  qp >= 0; chroma: the QP goes through kvz_get_scaled_qp first.
__host__ __device__ inline quant_consts flat_consts(int qp, int log2_tr, int chroma, int slice_is_intra, int signhide)
{
  const int quant_scales[6] = { 26214, 23302, 20560, 18396, 16384, 14564 };     // scalinglist.c:66
  const int inv_quant_scales[6] = { 40, 45, 51, 57, 64, 72 };                   // scalinglist.c:67
  const int transform_shift = 15 - 8 - log2_tr;
  const int qps = scaled_qp(chroma ? 2 : 0, qp);
  quant_consts c;
  c.q_bits = 14 + qps / 6 + transform_shift;
  c.add = (slice_is_intra ? 171 : 85) << (c.q_bits - 9);
  c.flat_qc = quant_scales[qps % 6];
  c.signhide = signhide;
  c.qtable = nullptr;
  c.dq_mode = 0; c.dqtable = nullptr;
  c.dq_scale = inv_quant_scales[qps % 6] << (qps / 6);
  c.dq_shift = 20 - 14 - transform_shift; c.dq_add = 1 << (c.dq_shift - 1);
  return c;
}
// the LCU QP the per-LCU entries use: any value is brought into 0..51 (the reference's CLIP_TO_QP), so that no value leaves a table
__host__ __device__ inline int clip_lcu_qp(int qp) { return qp < 0 ? 0 : (qp > 51 ? 51 : qp); }

// The packed scaling lists of kvz_hip_scaling_tables (kvz_hip.h): where table (size_id, list, rem) begins in either array
__host__ __device__ constexpr int sl_table_offset(int size_id, int list, int rem)
{
  // 36 tables of every smaller size come first: 16 + 64 + .. = (16 * 4^size_id - 16) / 3 values each
  return 12 * ((16 << (2 * size_id)) - 16) + ((6 * list + rem) << (2 * size_id + 4));
}
// The constants of one TU under scaling lists, on the host and on the device: flat_consts with the table pointers, dq_mode and
// dq_shift / dq_add on top -- the arithmetic of make_consts below, for the whole-picture entries, which pick a TU's tables on the
// device from its size, its plane (0 Y, 1 U, 2 V), its CU's type and the QP of its LCU.  The reference quantises V with U's list
// (type 2, quant-generic.c:223 with :46-47) and dequantises each plane with its own (:244, :293-295); both branches of :296-311.
__host__ __device__ inline quant_consts sl_consts(int qp, int log2_tr, int plane, int cu_is_intra, int slice_is_intra, int signhide,
                                                  const int32_t *quant, const int32_t *dequant)
{
  quant_consts c = flat_consts(qp, log2_tr, plane != 0, slice_is_intra, signhide);
  const int qps = scaled_qp(plane ? 2 : 0, qp), base = cu_is_intra ? 0 : 3, shift = log2_tr + 3;
  c.qtable = quant + sl_table_offset(log2_tr - 2, base + (plane ? 1 : 0), qps % 6);
  c.dqtable = dequant + sl_table_offset(log2_tr - 2, base + plane, qps % 6);
  if (shift > qps / 6) { c.dq_mode = 1; c.dq_shift = shift - qps / 6; c.dq_add = 1 << (c.dq_shift - 1); }
  else { c.dq_mode = 2; c.dq_shift = qps / 6 - shift; c.dq_add = 0; }
  c.dq_scale = 0;
  return c;
}

// quant-generic.c:40-50 and :283-320: flat_consts, with the scaling-list tables on top where they are given
static bool make_consts(const kvz_hip_quant_params *p, int width, int type_q, int type_dq, quant_consts *c)
{
  if (width != 4 && width != 8 && width != 16 && width != 32) return false;
  const int log2_tr = log2i(width);
  if (scaled_qp(type_q, p->qp) < 0) return false;
  *c = flat_consts(p->qp, log2_tr, type_q != 0, p->slice_is_intra, p->signhide);
  c->qtable = (p->scaling_list && p->quant_coeff) ? p->quant_coeff : nullptr;
  if ((type_q != 0) != (type_dq != 0)) {
    const quant_consts d = flat_consts(p->qp, log2_tr, type_dq != 0, p->slice_is_intra, p->signhide);
    c->dq_scale = d.dq_scale; c->dq_shift = d.dq_shift; c->dq_add = d.dq_add;
  }
  if (p->scaling_list && p->dequant_coeff) {
    const int qps = scaled_qp(type_dq, p->qp);
    const int shift = c->dq_shift + 4;
    c->dqtable = p->dequant_coeff;
    if (shift > qps / 6) { c->dq_mode = 1; c->dq_shift = shift - qps / 6; c->dq_add = 1 << (c->dq_shift - 1); }
    else { c->dq_mode = 2; c->dq_shift = qps / 6 - shift; c->dq_add = 0; }
    c->dq_scale = 0;
  }
  return true;
}

// quant-generic.c:55-67: unsigned level before sign/clip
__device__ __forceinline__ int quant_level(int c, int qc, const quant_consts &k)
{
  const int a = c < 0 ? -c : c;
  // flat quantisation: |c| <= 2^15 and quant_scales < 2^15, so the product is a full-rate 24-bit multiply and the sum
  // stays below 2^31 (add < 2^26); only scaling lists need the reference's 64-bit product (v_mul_lo_u32 and the 64-bit
  // multiply-add run at a quarter of the rate)
  if (!k.qtable) return (int)((__umul24((unsigned)a, (unsigned)qc) + (unsigned)k.add) >> k.q_bits);
  return (int)(((long long)a * qc + k.add) >> k.q_bits);
}
__device__ __forceinline__ int quant_one(int c, int qc, const quant_consts &k)
{
  int level = quant_level(c, qc, k);
  level = c < 0 ? -level : level;
  return clip16(level);
}
// quant-generic.c:290-320
__device__ __forceinline__ int dequant_one(int q, int n, const quant_consts &k)
{
  if (k.dq_mode == 0) return clip16((int)((unsigned)__mul24(q, k.dq_scale) + (unsigned)k.dq_add) >> k.dq_shift);   // |q| <= 2^15, scale <= 72 << 8
  const int d = k.dqtable[n];
  if (k.dq_mode == 1) return clip16((q * d + k.dq_add) >> k.dq_shift);
  int v = clip16(q * d);
  return clip16((int)((unsigned)v << k.dq_shift));
}
// the same with the table entry d already loaded (the whole-picture kernels read their row of the table as 16-byte vectors);
// dq_mode is 1 or 2
__device__ __forceinline__ int dequant_listed(int q, int d, const quant_consts &k)
{
  if (k.dq_mode == 1) return clip16((q * d + k.dq_add) >> k.dq_shift);
  const int v = clip16(q * d);
  return clip16((int)((unsigned)v << k.dq_shift));
}
// quant_one with a table entry: always the reference's 64-bit product (quant-generic.c:62)
__device__ __forceinline__ int quant_listed(int c, int qc, const quant_consts &k)
{
  const int a = c < 0 ? -c : c;
  const int level = (int)(((long long)a * qc + k.add) >> k.q_bits);
  return clip16(c < 0 ? -level : level);
}

// kvz_get_coeff_cost below fast_residual_cost_limit (rdo.c:44-45, :219-220): (uint32_t)(sum * (qp * 0.044407704 + 0.557323653) + 0.5)
// in doubles.  The host rounds each multiply and each add; the intrinsics keep the compiler from contracting them into fused operations,
// which round once.
__device__ __forceinline__ u32 trskip_coeff_cost(u32 sum, int qp)
{
  return (u32)__dadd_rn(__dmul_rn((double)sum, __dadd_rn(__dmul_rn((double)qp, 0.044407704), 0.557323653)), 0.5);
}

// ---- sign bit hiding (quant-generic.c:69-162) on one block; coef/q_coef may be
// global or LDS pointers.  Sequential per block, exactly the reference's control
// flow (including `abssum` being a signed sum and `cur_change` persisting across
// iterations).  Only reached with --signhide (off at preset medium). ----
// position of scan index `idx` for (scan_idx, log2 size): kvz_g_sig_last_scan
// (tables.c): 4x4 coefficient groups, group order and in-group order both follow
// the pattern (0 up-right diagonal, 1 horizontal, 2 vertical).
__device__ __forceinline__ int pattern_pos4(int scan_idx, int i)     // i in 0..15 -> y*4 + x inside a 4x4
{
  if (scan_idx == 1) return i;
  if (scan_idx == 2) return ((i & 3) << 2) | (i >> 2);
  const unsigned char t[16] = { 0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15 };
  return t[i];
}
// order of the g x g groups (g = 1, 2, 4, 8): returns gy * g + gx of the i-th group
__device__ __forceinline__ int pattern_group(int scan_idx, int g, int i)
{
  if (scan_idx == 1) return i;
  if (scan_idx == 2) return (i % g) * g + (i / g);
  // up-right diagonal over a g x g grid: walk anti-diagonals from bottom-left to top-right
  int c = 0;
  for (int d = 0; d < 2 * g - 1; ++d) {
    const int y0 = d < g ? d : g - 1;
    const int cnt = (d < g) ? d + 1 : 2 * g - 1 - d;
    if (i < c + cnt) { const int y = y0 - (i - c); return y * g + (d - y); }
    c += cnt;
  }
  return 0;
}
__device__ __forceinline__ int scan_pos(int scan_idx, int log2_size, int idx)
{
  const int n = 1 << log2_size;
  if (log2_size == 2) return pattern_pos4(scan_idx, idx);
  const int g = n >> 2;
  const int grp = pattern_group(scan_idx, g, idx >> 4);
  const int p = pattern_pos4(scan_idx, idx & 15);
  return ((grp / g) * 4 + (p >> 2)) * n + (grp % g) * 4 + (p & 3);
}

// One coefficient group (16 coefficients in scan order, positions pos16) of the sign-hiding pass, quant-generic.c:82-156.
// A group reads and changes only its own coefficients; what it needs from the rest of the block is whether it is the
// "last" group -- the highest one in scan order that holds a non-zero level (last_cg, :99-101, :153).
template <typename CP, typename QP>
__device__ __forceinline__ void sign_hide_cg(CP coef, QP q_coef, const int (&pos16)[16], bool is_last_cg, const quant_consts &k)
{
  const int q_bits8 = k.q_bits - 8;
  auto delta_u = [&](int pos) -> int {
    const int qc = k.qtable ? k.qtable[pos] : k.flat_qc;
    const int c = coef[pos];
    const long long prod = (long long)(c < 0 ? -c : c) * qc;
    const int level = (int)((prod + k.add) >> k.q_bits);
    return (int)((prod - (long long)(int)((unsigned)level << k.q_bits)) >> q_bits8);
  };
  int first_nz = 16, last_nz = -1, abssum = 0;
  for (int n = 15; n >= 0; --n) if (q_coef[pos16[n]]) { last_nz = n; break; }
  for (int n = 0; n < 16; ++n) if (q_coef[pos16[n]]) { first_nz = n; break; }
  for (int n = first_nz; n <= last_nz; ++n) abssum += q_coef[pos16[n]];
  if (last_nz - first_nz < 4) return;
  const int signbit = q_coef[pos16[first_nz]] > 0 ? 0 : 1;
  if (signbit == (abssum & 1)) return;
  int min_cost_inc = 0x7fffffff, min_pos = -1, cur_cost = 0x7fffffff;
  int final_change = 0, cur_change = 0;
  for (int n = (is_last_cg ? last_nz : 15); n >= 0; --n) {
    const int pos = pos16[n];
    const int q = q_coef[pos];
    if (q != 0) {
      const int du = delta_u(pos);
      if (du > 0) { cur_cost = -du; cur_change = 1; }
      else if (n == first_nz && (q == 1 || q == -1)) { cur_cost = 0x7fffffff; }
      else { cur_cost = du; cur_change = -1; }
    } else if (n < first_nz && ((coef[pos] >= 0) ? 0 : 1) != signbit) {
      cur_cost = 0x7fffffff;
    } else { cur_cost = -delta_u(pos); cur_change = 1; }
    if (cur_cost < min_cost_inc) { min_cost_inc = cur_cost; final_change = cur_change; min_pos = pos; }
  }
  const int qm = q_coef[min_pos];
  if (qm == 32767 || qm == -32768) final_change = -1;
  if (coef[min_pos] >= 0) q_coef[min_pos] = (i16)(qm + final_change);
  else q_coef[min_pos] = (i16)(qm - final_change);
}

// the whole block on one thread, groups from the last to the first like the reference (used inside the fused kernel)
template <typename CP, typename QP>
__device__ void sign_hide_block(CP coef, QP q_coef, int width, int scan_idx, const quant_consts &k)
{
  const int log2_size = width == 4 ? 2 : width == 8 ? 3 : width == 16 ? 4 : 5;
  const int n_coef = width * width;
  unsigned ac_sum = 0;
  for (int n = 0; n < n_coef; ++n) ac_sum += (unsigned)quant_level(coef[n], k.qtable ? k.qtable[n] : k.flat_qc, k);
  if (ac_sum < 2) return;
  bool seen_nz = false;
  for (int subset = (n_coef - 1) >> 4; subset >= 0; --subset) {
    int pos16[16];
    bool nz = false;
#pragma unroll
    for (int n = 0; n < 16; ++n) { pos16[n] = scan_pos(scan_idx, log2_size, (subset << 4) + n); nz = nz || q_coef[pos16[n]] != 0; }
    sign_hide_cg(coef, q_coef, pos16, nz && !seen_nz, k);
    seen_nz = seen_nz || nz;
  }
}

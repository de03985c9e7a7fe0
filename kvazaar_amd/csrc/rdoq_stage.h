// rdoq_stage.h -- what the callers of rdoq_core.h share: the constants of one TU with the offset of its two tables, the nine state
// bytes by index (rdoq.hip and the stages), and RDOQ of one TU by one wave inside a stage of the picture chain (inter_residual_rdoq.hip,
// intra_recon_rdoq.hip): the body of rdoq_large_kernel on coefficients that already lie in LDS rows.  Device only; the translation
// units that include it are compiled with -ffp-contract=off (Makefile).
#pragma once
#include "rdoq_core.h"
#include "quant_core.h"

#pragma clang fp contract(off)

namespace kvzhip {

// byte i of the nine context bytes rdoq_core.h reads of a state (RQ_ROOT_CBF, RQ_CBF_LUMA.., RQ_CBF_CHROMA..), field by field
__device__ __forceinline__ u8 rdoq_state_byte(const kvz_hip_rdoq_state &st, int i)
{
  return i == RQ_ROOT_CBF ? st.root_cbf : i < RQ_CBF_CHROMA ? st.qt_cbf_luma[i - RQ_CBF_LUMA] : st.qt_cbf_chroma[i - RQ_CBF_CHROMA];
}

// the constants of one TU (rdo.c:553-564) and where its two tables begin
__device__ __forceinline__ rdoq_tu rdoq_make_tu(const kvz_hip_rdoq_desc &d, int qp, double lambda, int signhide, int &table_at)
{
  rdoq_tu t;
  t.log2w = d.width == 4 ? 2 : d.width == 8 ? 3 : d.width == 16 ? 4 : 5;
  t.type = d.type;
  t.scan_mode = d.scan_mode;
  t.intra = d.block_type == 1;
  t.tr_depth = d.tr_depth;
  t.qp_scaled = scaled_qp(d.type, qp);
  t.q_bits = 14 + t.qp_scaled / 6 + (15 - 8 - t.log2w);
  t.signhide = signhide;
  t.lambda = lambda;
  table_at = sl_table_offset(t.log2w - 2, (t.intra ? 0 : 3) + (d.type ? 1 : 0), t.qp_scaled % 6);
  return t;
}

}  // namespace kvzhip

#include "frame_sources.h"

namespace {

// ---- RDOQ inside a stage: one wave, one TU at a time, on the stage's rdoq_source (frame_sources.h) ----
// The wave's LDS: the arrays of the recursion for 1024 positions (rdoq_mem<1>), the TU's coefficients and levels dense, and the
// context set and state bytes of the wave's LCU.  About 50 KB.
struct rdoq_lds {
  double c0[1024], cc[1024], cs[1024], cg[64];
  i32 ld[1024], sig[1024], inc[1024], dec[1024], qd[1024], lx[12], ly[12];
  alignas(8) i16 dst[1024], coef[1024];
  double lambda;
  u8 ctx[CC_CTX_USED + 2], state[RQ_STATE_CTX + 3];
};

// the set of LCU `lcu`: an index beyond the table is its last set (the rule of kvz_hip_coeff_pricing)
__device__ __forceinline__ u32 rdoq_set_of(const rdoq_source &r, size_t lcu)
{
  const u32 want = r.lcu_ctx ? (u32)r.lcu_ctx[lcu] : 0u;
  return min(want, r.n_sets - 1u);
}

// the context bytes, the state bytes and lambda of set `set` into the wave's LDS; the wave's earlier reads of them are done
__device__ __forceinline__ void rdoq_stage_set(rdoq_lds &m, const rdoq_source &r, u32 set, int lane)
{
  const kvz_hip_coeff_ctx &c = r.sets[set];
  const kvz_hip_rdoq_state &st = r.states[set];
  wave_lds_fence();
  for (int k = lane; k < CC_CTX_USED - 2; k += 64) m.ctx[k] = c.ctx[k];
  if (lane < RQ_STATE_CTX) m.state[lane] = rdoq_state_byte(st, lane);
  if (lane == 0) m.lambda = st.lambda;
  wave_lds_fence();
}

// tr_depth as kvz_quantize_residual hands it to kvz_rdoq (quant-generic.c:218-219), from the first dword of the record at the TU's
// own top-left SCU, clamped into 0..3
__device__ __forceinline__ int rdoq_tr_depth(u32 head)
{
  const int depth = (head >> 8) & 255, part = (head >> 16) & 255, trd = (int)(head >> 24);
  const int d = trd - depth + (part == 3 ? 1 : 0);                  // SIZE_NxN (cu.h:49)
  return d < 0 ? 0 : (d > 3 ? 3 : d);
}

// kvz_rdoq of the N x N TU whose coefficients lie in the LDS rows `from` (LD values apart); the levels go to the rows `to`.  Called by
// all 64 lanes of a one-wave workgroup under wave-uniform conditions; the caller's writes of `from` are fenced here and the levels are
// visible to every lane on return.  qp: the QP of the TU's LCU, 0..51.  m holds the set staged by rdoq_stage_set.
template <int N, int LD>
__device__ __forceinline__ void rdoq_stage_tu(rdoq_lds &m, const rdoq_source &r, const i16 *from, i16 *to, int lane, int type, int scan_mode,
                                              int block_type, int tr_depth, int qp, int signhide)
{
  constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5, N2 = N * N;
  const rdoq_mem<1> mem = { m.c0, m.cc, m.cs, m.cg, m.ld, m.sig, m.inc, m.dec, m.qd, m.lx, m.ly, m.dst, m.coef };
  const rdoq_ctx ctx = { m.ctx, m.state };
  wave_lds_fence();
  for (int i = lane; i < N2; i += 64) m.coef[i] = from[(i >> LOG2) * LD + (i & (N - 1))];
  const kvz_hip_rdoq_desc d = { 0u, 0u, (u8)N, (u8)type, (u8)scan_mode, (u8)block_type, (u8)tr_depth, 0, 0 };
  int table_at;
  const rdoq_tu t = rdoq_make_tu(d, qp, m.lambda, signhide, table_at);
  const i32 *quant = r.quant + table_at;
  const double *err_scale = r.err_scale + table_at;
  const rdoq_scan sc = rdoq_make_scan(LOG2, scan_mode);
  wave_lds_fence();
  // per scan position: level_double, cost_coeff0, and the last position whose max_abs_level is above 0 (rdo.c:621-642)
  int last_scanpos = -1;
  for (int s0 = 0; s0 < N2; s0 += 64) {
    const int s = s0 + lane;
    bool some = false;
    if (s < N2) {
      const int blk = sc.blk(s);
      some = rdoq_prepare(mem, blk, quant[blk], err_scale[blk], t.q_bits) > 0;
    }
    const unsigned long long mask = __ballot(some);
    if (mask) last_scanpos = s0 + 63 - __clzll((long long)mask);
  }
  wave_lds_fence();
  int best = 0;
  if (last_scanpos >= 0) {
    if (lane == 0) best = rdoq_recursion(mem, ctx, sc, t, err_scale, last_scanpos);
    best = __builtin_amdgcn_readfirstlane(best);
    wave_lds_fence();
  }
  // signs and clean-up (rdo.c:866-876); abs_sum matters only as "at least 2"
  u32 abs_sum = 0;
  for (int s0 = 0; s0 < N2; s0 += 64) {
    const int s = s0 + lane;
    if (s < N2) {
      const u32 level = rdoq_finish(mem, sc.blk(s), s, best);
      abs_sum += level > 2 ? 2 : level;
    }
  }
  const unsigned long long ones = __ballot(abs_sum == 1), more = __ballot(abs_sum >= 2);
  wave_lds_fence();
  if (t.signhide && (more || __popcll(ones) >= 2)) {
    const int last_cg = (best - 1) >> 4;
    if (lane <= last_cg) rdoq_sign_hide_group(mem, sc, lane, last_cg, rdoq_rd_factor(t.qp_scaled, t.lambda));
    wave_lds_fence();
  }
  for (int i = lane; i < N2; i += 64) to[(i >> LOG2) * LD + (i & (N - 1))] = m.dst[i];
  wave_lds_fence();
}

// what a wave of a stage holds about its LCU: the source, the LCU's QP and set in LDS, sign hiding.  qp: the value the stage quantises
// the LCU's TUs with
template <> struct rdoq_lcu<true> {
  static constexpr bool on = true;
  typedef rdoq_lds lds;
  rdoq_lds *m;
  rdoq_source r;
  int qp, signhide;
  // whether a TU of width n takes RDOQ: width > 4 || !cfg.rdoq_skip (quant-generic.c:214)
  __device__ __forceinline__ bool takes(int n) const { return n > 4 || !r.skip; }
  __device__ __forceinline__ int tr_depth_of(u32 head) const { return rdoq_tr_depth(head); }
  __device__ __forceinline__ void stage(size_t lcu, int lane) const { rdoq_stage_set(*m, r, (u32)__builtin_amdgcn_readfirstlane(rdoq_set_of(r, lcu)), lane); }
  template <int N, int LD>
  __device__ __forceinline__ void tu(const i16 *from, i16 *to, int lane, int type, int scan_mode, int block_type, int tr_depth) const
  {
    rdoq_stage_tu<N, LD>(*m, r, from, to, lane, type, scan_mode, block_type, tr_depth, qp, signhide);
  }
};

}  // namespace

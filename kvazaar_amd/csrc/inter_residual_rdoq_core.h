// inter_residual_rdoq_core.h -- the kernel of the inter stage with RDOQ, a wave per TU: inter_residual_rdoq.hip instantiates it for one
// picture, inter_residual_multi_rdoq.hip for the table of per-picture records.  The algorithm is described in
// inter_residual_rdoq.hip.  Device only; the translation units that include it are compiled with -ffp-contract=off (Makefile).
#pragma once
#include "rdoq_stage.h"
#include "inter_residual_core.h"

#pragma clang fp contract(off)

namespace {

// One picture of kvz_hip_inter_residual_frames_rdoq: resid_pic, the picture's scaling tables, and its own context sets, states and
// set index per LCU.  184 bytes.  The RDOQ tables and rdoq_skip are the call's, once beside the records.
struct resid_pic_rdoq : resid_pic {
  const int32_t *quant, *dequant;          // SL: the packed tables
  const kvz_hip_coeff_ctx *sets;
  const kvz_hip_rdoq_state *states;
  const uint16_t *lcu_ctx;                 // or nullptr: set 0 in every LCU
  u32 n_sets, pad2;
};
struct resid_batch_rdoq {
  resid_pic_rdoq p[KVZ_HIP_MAX_CHAIN_PICTURES];
  const int32_t *quant;                    // kvz_hip_rdoq_tables of the call
  const double *err_scale;
  int skip, pad;
};
static_assert(sizeof(resid_pic_rdoq) == 184 && sizeof(resid_batch_rdoq) <= 3072, "the records travel in the kernel arguments");

template <typename ARGS> struct rdoq_batch_of { static constexpr bool multi = false; };
template <> struct rdoq_batch_of<resid_batch_rdoq> { static constexpr bool multi = true; };
// a COPY of the picture's block, as picture_of (inter_residual_core.h) and for its reasons
__device__ __forceinline__ resid_args rdoq_picture_of(const resid_args &a) { return a; }
__device__ __forceinline__ resid_pic_rdoq rdoq_picture_of(const resid_batch_rdoq &b) { return b.p[blockIdx.y]; }

// One slot per workgroup, one wave.  t: the lists (SL) and the QP of every LCU where q.lcu_qp is NULL.
// Several pictures (ARGS = resid_batch_rdoq, kvz_hip_inter_residual_frames_rdoq): grid (slots of the picture with the most, pictures);
// the wave takes its picture's record at blockIdx.y, counts that picture's slots itself and makes q, t and r of the record and the
// call's tables (the four counts and the three sources are not read as they come): a slot beyond its picture's count leaves at once.
template <int N, bool SL, typename ARGS>
__global__ __launch_bounds__(64) void inter_residual_rdoq_kernel(ARGS args, int nx_y, int n_y, int nx_c, int n_c, lcu_qp_source q, sl_source t,
                                                                 rdoq_source r)
{
  constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5, LD = lds_tile_ld(N), W4 = N / 4;
  __shared__ __attribute__((aligned(16))) i16 ta[N * LD];           // residual / coefficients
  __shared__ __attribute__((aligned(16))) i16 tb[N * LD];           // transform scratch
  __shared__ __attribute__((aligned(16))) i16 tq[N * LD];           // levels
  __shared__ rdoq_lds s_rdoq;

  const auto a = rdoq_picture_of(args);                             // the call's picture, or this wave's
  if constexpr (rdoq_batch_of<ARGS>::multi) {
    nx_y = (a.width + N - 1) / N; n_y = nx_y * ((a.height + N - 1) / N);
    nx_c = ((a.width >> 1) + N - 1) / N; n_c = (a.chroma && N < 32) ? nx_c * (((a.height >> 1) + N - 1) / N) : 0;
    q = { a.lcu_qp, a.slice_is_intra, a.signhide };
    t = { a.quant, a.dequant, a.qp };
    r = { a.sets, a.states, a.lcu_ctx, args.quant, args.err_scale, a.n_sets, args.skip };
  }
  // everything up to `own` is the same in every lane: the lanes beyond N repeat row lane % N, as in intra_tu
  const int lane = threadIdx.x, row = lane & (N - 1);
  const int slot = blockIdx.x;
  int plane = 0, lx = 0, ly = 0, cu_x = 0, cu_y = 0, leaf = 0;
  if (slot >= n_y + 2 * n_c) return;
  if (slot < n_y) {
    const int ty = slot / nx_y;
    lx = N * (slot - ty * nx_y);
    ly = N * ty;
  } else {
    int s = slot - n_y;
    plane = 1;
    if (s >= n_c) { s -= n_c; plane = 2; }
    const int ty = s / nx_c;
    lx = 2 * N * (s - ty * nx_c);
    ly = 2 * N * ty;
  }
  if (lx >= a.width || ly >= a.height || !inter_cu_at(a, lx, ly, cu_x, cu_y, leaf)) return;
  // chroma TUs are half as wide; with 4x4 luma TUs the chroma of the 8x8 area is one 4x4 TU (transform.c:293-313)
  if (!(plane == 0 ? leaf == N : (N == 4 ? leaf <= 8 : leaf == 2 * N))) return;

  const size_t lcu = (size_t)(ly >> 6) * a.lcus_x + (lx >> 6);
  // the QP of the entry without RDOQ: the array's value clamped; without an array the lists' entry clamps the picture's QP and the
  // flat one takes it as it stands (the host has refused what make_consts refuses)
  int qp = q.lcu_qp ? clip_lcu_qp((int)q.lcu_qp[lcu]) : (SL ? clip_lcu_qp(t.qp) : t.qp);
  qp = (int)__builtin_amdgcn_readfirstlane((u32)qp);
  quant_consts k;
  if constexpr (SL) k = sl_consts(qp, LOG2, plane, 0, q.slice_is_intra, q.signhide, t.quant, t.dequant);
  else k = flat_consts(qp, LOG2, plane, q.slice_is_intra, q.signhide);

  const bool own = lane < N;                                        // the lanes that touch global memory
  const int sh = plane ? 1 : 0, px = lx >> sh, py = ly >> sh;
  const u8 *src_row = (plane == 0 ? a.src_y : (plane == 1 ? a.src_u : a.src_v)) + (size_t)(py + row) * (plane ? a.src_stride_c : a.src_stride_y) + px;
  u8 *rec_row = (plane == 0 ? a.rec_y : (plane == 1 ? a.rec_u : a.rec_v)) + (size_t)(py + row) * (plane ? a.rec_stride_c : a.rec_stride_y) + px;
  u32 sw[W4], pw[W4];
  load_row<N>(src_row, sw);
  load_row<N>(rec_row, pw);
  u32 zssd = 0;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    const int d = byte_of(sw, x) - byte_of(pw, x);
    ta[row * LD + x] = (i16)d;
    zssd += (u32)(d * d);
  }
  __syncthreads();
  transform_2d_lds<N, 0, LD>(ta, tb, row);
  __syncthreads();
  int any = 0;
  if (N > 4 || !r.skip) {
    // kvz_rdoq: type 0 / 2, the diagonal scan of an inter CU, block_type CU_INTER, tr_depth of the record at the TU's top-left SCU
    const u32 head = __builtin_amdgcn_readfirstlane(a.cus[((size_t)(ly >> 2) * a.cus_stride + (lx >> 2)) * 5]);
    rdoq_stage_set(s_rdoq, r, (u32)__builtin_amdgcn_readfirstlane(rdoq_set_of(r, lcu)), lane);
    rdoq_stage_tu<N, LD>(s_rdoq, r, ta, tq, lane, plane ? 2 : 0, 0, 2, rdoq_tr_depth(head), clip_lcu_qp(qp), q.signhide != 0);
  } else {
    if constexpr (SL) {
#pragma unroll
      for (int x = 0; x < N; ++x) tq[row * LD + x] = (i16)quant_listed(ta[row * LD + x], k.qtable[row * N + x], k);
    } else {
#pragma unroll
      for (int x = 0; x < N; ++x) tq[row * LD + x] = (i16)quant_one(ta[row * LD + x], k.flat_qc, k);
    }
    if (k.signhide) {
      __syncthreads();
      if (lane == 0) {
        struct lds_view { i16 *p; int ld, n; __device__ i16 &operator[](int i) const { return p[(i / n) * ld + (i % n)]; } };
        lds_view cv = { ta, LD, N }, qv = { tq, LD, N };
        sign_hide_block(cv, qv, N, 0, k);                                       // diagonal: kvz_get_scan_order of an inter CU
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int x = 0; x < N; ++x) any |= tq[row * LD + x];
  const int has = __syncthreads_or(any) ? 1 : 0;
  u32 sab = 0;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    const int l = tq[row * LD + x];
    sab += (u32)(l < 0 ? -l : l);
    if constexpr (SL) ta[row * LD + x] = (i16)dequant_listed(l, k.dqtable[row * N + x], k);
    else ta[row * LD + x] = (i16)dequant_one(l, row * N + x, k);
  }
  __syncthreads();
  transform_2d_lds<N, 1, LD>(ta, tb, row);
  __syncthreads();
  u32 ssd = zssd;                                    // a TU without coefficients keeps its prediction (quant-generic.c:262-271)
  if (has) {
    u32 ow[W4];
    ssd = 0;
#pragma unroll
    for (int j = 0; j < W4; ++j) {
      u32 o = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = 4 * j + i;
        const i16 val = (i16)((int)ta[row * LD + x] + byte_of(pw, x));             // quant-generic.c:255
        const int c = val < 0 ? 0 : (val > 255 ? 255 : val);
        const int d = byte_of(sw, x) - c;
        ssd += (u32)(d * d);
        o |= (u32)c << (8 * i);
      }
      ow[j] = o;
    }
    if (own) store_row<N>(rec_row, ow);
  }
  if (own) {
    const int bx = (lx & 63) >> (2 + sh), by = (ly & 63) >> (2 + sh);
    i16 *dst = (plane == 0 ? a.coeff_y : (plane == 1 ? a.coeff_u : a.coeff_v)) + lcu * (plane ? 1024 : 4096) + 16 * zorder_blk(bx, by) + row * N;
    if (N == 4) {
      *(uint2 *)dst = make_uint2(*(const u32 *)(tq + row * LD), *(const u32 *)(tq + row * LD + 2));
    } else {
#pragma unroll
      for (int j = 0; j < N / 8; ++j) *(uint4 *)(dst + 8 * j) = lds_tile_load8<N, LD>(tq, row * N + 8 * j);
    }
    // flags of the SCUs the TU covers: cbf_y as lcu_set_coeff leaves it (search.c:173-190), bit `plane` of cbf_out
    const int sx0 = lx >> 2, sy0 = ly >> 2;
    if (plane == 0) {
      if ((row & 3) == 0) {
        for (int i = 0; i < W4; ++i) {
          const size_t scu = (size_t)(sy0 + (row >> 2)) * a.cus_stride + sx0 + i;
          ((u8 *)a.cus)[scu * 20 + 4] = (u8)has;
          if (a.cbf_out && has) or_byte(a.cbf_out, scu, 1u);
        }
      }
    } else if (row < N / 2 && a.cbf_out && has) {
      for (int i = 0; i < N / 2; ++i) or_byte(a.cbf_out, (size_t)(sy0 + row) * a.cus_stride + sx0 + i, 1u << plane);
    }
  }
  if (a.cost) {
    // the inputs of the CU's cost (search.c:580-642): integer sums, so the order of the additions does not matter
    ssd = group_sum<64>(own ? ssd : 0u);
    zssd = group_sum<64>(own ? zssd : 0u);
    sab = group_sum<64>(own ? sab : 0u);
    if (lane == 0) {
      u32 *c = a.cost + ((size_t)(cu_y >> 2) * a.cus_stride + (cu_x >> 2)) * 6 + sh;
      atomicAdd(c, ssd);
      atomicAdd(c + 2, zssd);
      atomicAdd(c + 4, sab);
    }
  }
}

}  // namespace

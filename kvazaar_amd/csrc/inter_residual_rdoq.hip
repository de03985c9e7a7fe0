// inter_residual_rdoq.hip -- kvz_hip_inter_residual_frame_rdoq: kvz_hip_inter_residual_frame_sl (inter_residual_sl.hip) with the quantiser
// of the reference at preset medium and slower: a TU wider than 4, and a 4x4 TU unless cfg.rdoq_skip, takes its levels from kvz_rdoq
// (quant-generic.c:214-221) on the context set and the state of its LCU.  The arrays of kvz_rdoq's recursion take about 50 KB of LDS
// per TU (rdoq_stage.h), so the 256 / N TUs of a workgroup of inter_residual_tu_kernel do not fit: the kernel here gives a TU a wave
// of its own, in the manner of the quantise half of intra_tu (intra_recon_core.h).  The slots, the CU rule, the constants of a TU,
// the coefficient layout, the flags and the sums are those of inter_residual_tu_kernel; a slot that is no TU leaves at once.  Between
// the forward transform and the has-coefficients flag the wave runs the body of rdoq_large_kernel: level_double across the lanes,
// last_scanpos by a ballot, the recursion on lane 0, clean-up and sign hiding across the lanes.  With rdoq_skip the 4x4 launch is the
// instantiation of inter_residual_tu_kernel that the entry without RDOQ launches.  This translation unit is compiled with
// -ffp-contract=off (Makefile), as rdoq.hip is.
#include "rdoq_stage.h"
#include "inter_residual_core.h"

#pragma clang fp contract(off)

namespace {

// One slot per workgroup, one wave.  t: the lists (SL) and the QP of every LCU where q.lcu_qp is NULL.
template <int N, bool SL>
__global__ __launch_bounds__(64) void inter_residual_rdoq_kernel(resid_args a, int nx_y, int n_y, int nx_c, int n_c, lcu_qp_source q, sl_source t,
                                                                 rdoq_source r)
{
  constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5, LD = lds_tile_ld(N), W4 = N / 4;
  __shared__ __attribute__((aligned(16))) i16 ta[N * LD];           // residual / coefficients
  __shared__ __attribute__((aligned(16))) i16 tb[N * LD];           // transform scratch
  __shared__ __attribute__((aligned(16))) i16 tq[N * LD];           // levels
  __shared__ rdoq_lds s_rdoq;

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

template <int N, bool SL>
void launch_rdoq_size(const resid_args &a, int chroma, hipStream_t st, const lcu_qp_source &q, const sl_source &t, const rdoq_source &r)
{
  const resid_slots n = residual_slots<N>(a.width, a.height, chroma);
  hipLaunchKernelGGL((inter_residual_rdoq_kernel<N, SL>), dim3((unsigned)(n.n_y + 2 * n.n_c)), dim3(64), 0, st, a, n.nx_y, n.n_y, n.nx_c, n.n_c, q, t, r);
}

// the record checked as residual_frame checks it; one launch per size, 32 down to 4, behind the init kernel
template <bool SL>
int residual_rdoq_frame(const char *entry, const kvz_hip_chain_picture &p, const kvz_hip_scaling_tables *tables, const rdoq_source &r, kvz_hip_stream s)
{
  if (!chain_picture_args_ok(p, false, SL) || (SL && !chain_tables_ok(*tables)) || !chain_one_qp_ok(p)) return kvzhip::invalid_arg(entry);
  const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
  const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
  quant_consts ky = {}, kc = {};                                              // read by the 4x4 kernel without a trailing source only
  if (!SL && !p.lcu_qp) {
    // one QP and flat lists: what the one-QP entry refuses (make_consts per size, quant_core.h)
    for (int n = 32; n >= 4; n >>= 1)
      if (!make_consts(&qp, n, 0, 0, &ky) || !make_consts(&qp, n, 2, 2, &kc)) return kvzhip::invalid_arg(entry);
  }
  resid_args a;
  a.src_y = p.src.y; a.src_u = chroma ? p.src.u : nullptr; a.src_v = chroma ? p.src.v : nullptr;
  a.rec_y = p.rec_y; a.rec_u = chroma ? p.rec_u : nullptr; a.rec_v = chroma ? p.rec_v : nullptr;
  a.src_stride_y = p.src.stride_y; a.src_stride_c = p.src.stride_c; a.rec_stride_y = p.stride_y; a.rec_stride_c = p.stride_c;
  a.coeff_y = p.coeff_y; a.coeff_u = chroma ? p.coeff_u : nullptr; a.coeff_v = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs;
  a.cus_stride = width >> 2; a.lcus_x = (width + 63) >> 6;
  a.width = width; a.height = height;
  hipStream_t st = ctx_stream(s);
  if (p.cbf_out || p.costs) {
    const int n_scu = (width >> 2) * (height >> 2);
    hipLaunchKernelGGL(inter_residual_init_kernel, dim3((unsigned)((n_scu + 255) / 256)), dim3(256), 0, st, a, n_scu);
    KVZ_CHECK_LAUNCH("inter_residual_init_kernel");
  }
  const lcu_qp_source per_lcu = qp_source_of(p);
  const sl_source lists = { SL ? tables->quant : nullptr, SL ? tables->dequant : nullptr, p.params.qp };
  launch_rdoq_size<32, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_size<16, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  launch_rdoq_size<8, SL>(a, chroma, st, per_lcu, lists, r);
  KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  if (!r.skip) {
    launch_rdoq_size<4, SL>(a, chroma, st, per_lcu, lists, r);
    KVZ_CHECK_LAUNCH("inter_residual_rdoq_kernel");
  } else {
    // every 4x4 TU keeps the plain quantiser: the 4x4 launch of the entry without RDOQ
    if constexpr (SL) launch_size<4>(a, ky, kc, chroma, st, per_lcu, lists);
    else if (p.lcu_qp) launch_size<4>(a, ky, kc, chroma, st, per_lcu);
    else launch_size<4>(a, ky, kc, chroma, st);                              // ky, kc: make_consts of size 4, the last made above
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_inter_residual_frame_rdoq(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                      kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                      kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                      const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables, const kvz_hip_rdoq_source *rdoq,
                                      const kvz_hip_inter_residual_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!rdoq) {
    // without it, it is the entry without it, launching that entry's kernels
    return kvz_hip_inter_residual_frame_sl(src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, coeff_y, coeff_u, coeff_v, cbf_out, costs, lcu_qp, tables,
                                           params, s);
  }
  if (const char *why = chain_rdoq_why(rdoq)) {
    char msg[200];
    snprintf(msg, sizeof msg, "invalid argument (%s)", why);
    return refuse_entry(__func__, msg);
  }
  kvz_hip_chain_picture p;
  const bool packed = chain_picture_pack(&p, src, rec_y, stride_y, rec_u, rec_v, stride_c, cus, nullptr, coeff_y, coeff_u, coeff_v, cbf_out, costs,
                                         lcu_qp, params);
  if (!packed) return kvzhip::invalid_arg(__func__);
  const rdoq_source rq = { rdoq->ctx_sets, rdoq->states, rdoq->lcu_ctx, rdoq->tables.quant, rdoq->tables.err_scale, rdoq->n_sets, rdoq->rdoq_skip != 0 };
  // without tables, what the _sl entry refuses without them is refused: scaling_list says whether tables are given
  if (tables) return residual_rdoq_frame<true>(__func__, p, tables, rq, s);
  return residual_rdoq_frame<false>(__func__, p, nullptr, rq, s);
}

}  // extern "C"

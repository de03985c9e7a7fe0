// inter_residual_core.h -- the kernels and the host side of the whole-picture inter residual entries (inter_residual.hip: one QP per
// call and a QP per LCU; inter_residual_sl.hip: scaling lists; inter_residual_ts.hip: transform skip; inter_residual_multi.hip: several pictures in one call;
// inter_residual_multi_ts.hip: several pictures with scaling lists and transform skip; through inter_residual_rdoq_core.h the two RDOQ
// units, which take the fill of resid_args, the init launch and the 4x4 launch of rdoq_skip from here).  Everything here has internal
// linkage: each translation unit gets its own copy and instantiates its own kernels.  The algorithm is described in inter_residual.hip.
#pragma once

#include "kvz_hip_internal.h"
#include "transform_core.h"
#include "quant_core.h"
#include "lcu_layout.h"
#include "frame_sources.h"
#include "chain_host.h"
#include "coeff_cabac_core.h"

using namespace kvzhip;

namespace {

static_assert(sizeof(kvz_hip_inter_residual_params) == 24 && sizeof(kvz_hip_inter_residual_cost) == 24 && sizeof(kvz_hip_cu_info) == 20,
              "layouts documented in kvz_hip.h");

struct resid_args {
  const u8 *src_y, *src_u, *src_v;
  u8 *rec_y, *rec_u, *rec_v;
  u32 src_stride_y, src_stride_c, rec_stride_y, rec_stride_c;
  i16 *coeff_y, *coeff_u, *coeff_v;
  u32 *cus;                      // records as five dwords; cbf_y is byte 4
  u8 *cbf_out;                   // or nullptr
  u32 *cost;                     // six dwords per SCU, or nullptr
  int cus_stride, lcus_x;
  int width, height;
};
// a checked record into the arguments of the single-picture kernels
inline void fill(resid_args &a, const kvz_hip_chain_picture &p)
{
  const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
  a.src_y = p.src.y; a.src_u = chroma ? p.src.u : nullptr; a.src_v = chroma ? p.src.v : nullptr;
  a.rec_y = p.rec_y; a.rec_u = chroma ? p.rec_u : nullptr; a.rec_v = chroma ? p.rec_v : nullptr;
  a.src_stride_y = p.src.stride_y; a.src_stride_c = p.src.stride_c; a.rec_stride_y = p.stride_y; a.rec_stride_c = p.stride_c;
  a.coeff_y = p.coeff_y; a.coeff_u = chroma ? p.coeff_u : nullptr; a.coeff_v = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs;
  a.cus_stride = width >> 2; a.lcus_x = (width + 63) >> 6;
  a.width = width; a.height = height;
}

// One picture of a multi-picture call (kvz_hip_inter_residual_frames): resid_args under the same member names, and what a TU derives
// its constants from (flat_consts with lcu_qp[] or qp, as the per-LCU kernel).  136 bytes; sixteen of them are the kernel's argument,
// and a workgroup reads its own at blockIdx.y: every address is wave-uniform and in the kernel-argument segment, so the fields come
// through scalar loads into scalar registers.
struct resid_pic {
  const u8 *src_y, *src_u, *src_v;
  u8 *rec_y, *rec_u, *rec_v;
  i16 *coeff_y, *coeff_u, *coeff_v;
  u32 *cus;
  u8 *cbf_out;                   // or nullptr
  u32 *cost;                     // or nullptr
  const int8_t *lcu_qp;          // or nullptr: qp in every LCU
  u32 src_stride_y, src_stride_c, rec_stride_y, rec_stride_c;
  int qp;
  uint16_t width, height, cus_stride, lcus_x;      // a picture is at most 16384 wide and high
  u8 chroma, slice_is_intra, signhide, pad;
};
struct resid_batch { resid_pic p[KVZ_HIP_MAX_CHAIN_PICTURES]; };
// a checked record into the kernel's; qp: the picture's QP as the kernel is to see it (as it stands, or clamped: the entries differ)
inline void fill(resid_pic &a, const kvz_hip_chain_picture &p, int qp)
{
  const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
  a.src_y = p.src.y; a.src_u = chroma ? p.src.u : nullptr; a.src_v = chroma ? p.src.v : nullptr;
  a.rec_y = p.rec_y; a.rec_u = chroma ? p.rec_u : nullptr; a.rec_v = chroma ? p.rec_v : nullptr;
  a.src_stride_y = p.src.stride_y; a.src_stride_c = p.src.stride_c; a.rec_stride_y = p.stride_y; a.rec_stride_c = p.stride_c;
  a.coeff_y = p.coeff_y; a.coeff_u = chroma ? p.coeff_u : nullptr; a.coeff_v = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
  a.qp = qp;
  a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
  a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
}
static_assert(sizeof(resid_pic) == 136 && sizeof(resid_batch) <= 3072, "the records travel in the kernel arguments");
// The kernel works on a COPY of its picture's block, which the compiler takes apart into the loads of the fields that are used: for
// resid_args that is the kernel as it was compiled with the argument itself, instruction for instruction, which a reference to the
// argument is not (tools/compare_kernels.py); for resid_pic they are scalar loads at an offset that blockIdx.y gives.
__device__ __forceinline__ resid_args picture_of(const resid_args &a) { return a; }
__device__ __forceinline__ resid_pic picture_of(const resid_batch &b) { return b.p[blockIdx.y]; }
// One picture of kvz_hip_inter_residual_frames_ts: resid_pic, then what the _sl and _ts entries take as trailing arguments.  176 bytes.
// The options that select an instantiation are the type of the table: a call is homogeneous in them.
struct resid_pic_ts : resid_pic {
  const int32_t *quant, *dequant;          // SL: the packed tables
  const int32_t *lcu_bit_cost;             // TS: or nullptr, bit_cost in every LCU
  u8 *tr_skip_out;                         // TS
  int bit_cost, pad2;
};
struct resid_batch_ts_data { resid_pic_ts p[KVZ_HIP_MAX_CHAIN_PICTURES]; };
template <bool SL, bool TS> struct resid_batch_ts : resid_batch_ts_data {};
static_assert(sizeof(resid_pic_ts) == 176 && sizeof(resid_batch_ts<true, true>) <= 3072, "the records travel in the kernel arguments");
template <bool SL, bool TS> __device__ __forceinline__ resid_pic_ts picture_of(const resid_batch_ts<SL, TS> &b) { return b.p[blockIdx.y]; }
// what the type of the kernel's first argument says about the instantiation
template <typename ARGS> struct batch_of { static constexpr bool multi = false, sl = false, ts = false; };
template <> struct batch_of<resid_batch> { static constexpr bool multi = true, sl = false, ts = false; };
template <bool SL, bool TS> struct batch_of<resid_batch_ts<SL, TS>> { static constexpr bool multi = true, sl = SL, ts = TS; };

// the inter CU that holds the luma position (x, y), from the record of that position alone: false for another type, a
// depth beyond 3 or a CU that would leave the picture (the rule of kvz_hip_inter_recon_frame)
template <typename ARGS>
__device__ __forceinline__ bool inter_cu_at(const ARGS &a, int x, int y, int &cu_x, int &cu_y, int &leaf)
{
  const u32 head = a.cus[((size_t)(y >> 2) * a.cus_stride + (x >> 2)) * 5];
  const int depth = (head >> 8) & 255, trd = (int)(head >> 24);
  if ((head & 255u) != 2u || depth > 3) return false;                         // CU_INTER (cu.h:38-43)
  const int size = 64 >> depth;
  cu_x = x & ~(size - 1);
  cu_y = y & ~(size - 1);
  // transform.c:448: split while depth == 0 or tr_depth > depth; 4x4 is the smallest TU
  leaf = 64 >> min(4, max(max(depth, trd), 1));
  return cu_x + size <= a.width && cu_y + size <= a.height;
}

// the rule as the init kernels ask it (zero_cu_outputs, frame_sources.h): the record is found from the position, as everywhere here
struct inter_cu_rule {
  template <typename PIC> __device__ __forceinline__ bool operator()(const PIC &a, int, int x, int y, int &cu_x, int &cu_y, int &leaf) const
  {
    return inter_cu_at(a, x, y, cu_x, cu_y, leaf);
  }
};

// cbf_out and costs start from zero inside the inter CUs
__global__ __launch_bounds__(256) void inter_residual_init_kernel(resid_args a, int n_scu)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_scu) return;
  zero_cu_outputs(a, i, inter_cu_rule());
}
// launched where the picture has one of the two outputs
inline int residual_init(const resid_args &a, hipStream_t st)
{
  if (!a.cbf_out && !a.cost) return KVZ_HIP_OK;
  const int n_scu = (a.width >> 2) * (a.height >> 2);
  hipLaunchKernelGGL(inter_residual_init_kernel, dim3((unsigned)((n_scu + 255) / 256)), dim3(256), 0, st, a, n_scu);
  KVZ_CHECK_LAUNCH("inter_residual_init_kernel");
  return KVZ_HIP_OK;
}

// The trailing sources of the kernel below (frame_sources.h), in their order.  The instantiations that an option adds have a
// translation unit of their own, so that those that were there before it compile to the code they were.
// A QP per LCU (kvz_hip_inter_residual_frame_qp, inter_residual.hip) is lcu_qp_source.  Every TU derives its own set from the QP of the
// LCU it lies in -- a workgroup holds 256 / N neighbouring slots of one row, up to four LCUs for N = 4, so the constants are per TU
// group, not per workgroup.  Without it (one QP per call) the instantiation is the kernel as it was, argument for argument.
// Scaling lists (kvz_hip_inter_residual_frame_sl, inter_residual_sl.hip) are a second trailing argument after the QP source: the two
// packed arrays, and the QP of every LCU where the source's array is NULL.  A TU's tables depend on its size, its plane and qp % 6 of
// its own LCU, so the pointers are per TU group like the rest of the constants (sl_consts, quant_core.h).
struct sl_source { const int32_t *quant, *dequant; int qp; };
// Transform skip (kvz_hip_inter_residual_frame_ts, inter_residual_ts.hip) comes after the QP source or after the lists, and only the
// N = 4 launch takes it: a luma slot runs kvz_quantize_residual twice, transformed and skipped, prices both and keeps the cheaper one
// (kvz_quantize_residual_trskip, transform.c:229-276).  qp: the QP of every LCU where the QP source's array is NULL and there are no
// lists.  Where the kernel takes no trailing argument (several pictures) it makes one of its picture's record.
struct ts_source { const int32_t *lcu_bit_cost; u8 *tr_skip_out; int bit_cost, qp; };
// CABAC pricing of the two trials (kvz_hip_inter_residual_frame_ts_cabac, inter_residual_ts_cabac.hip) is cabac_source, after the
// transform-skip source: the rule is applied per TU, each on a private copy of its LCU's context set, interleaved over the
// workgroup's TUs in LDS
template <int STRIDE> struct cabac_lds_ctx {
  u8 *p;
  __device__ __forceinline__ u32 get(int i) const { return p[i * STRIDE]; }
  __device__ __forceinline__ void set(int i, u32 v) { p[i * STRIDE] = (u8)v; }
};

// Slots: [0, n_y) the N-aligned positions of Y, nx_y per row; then n_c of U and n_c of V, nx_c per row (n_c = 0 for
// 4:0:0 and for N = 32).  A chroma slot (tx, ty) lies at the luma position (2 N tx, 2 N ty).
// Several pictures (ARGS = resid_batch, kvz_hip_inter_residual_frames): grid (workgroups of the picture with the most slots, pictures);
// the workgroup takes its picture's record at blockIdx.y, counts that picture's slots itself (ky, kc and the four counts are not read)
// and derives every TU's constants as the per-LCU kernel does.
template <int N, typename ARGS, typename... PER_LCU>
__global__ __launch_bounds__(256) void inter_residual_tu_kernel(ARGS args, quant_consts ky, quant_consts kc,
                                                                int nx_y, int n_y, int nx_c, int n_c, PER_LCU... per_lcu)
{
  constexpr bool MULTI = batch_of<ARGS>::multi, LCU_QP = MULTI || sizeof...(PER_LCU) != 0, SL = pack_has<sl_source, PER_LCU...> || batch_of<ARGS>::sl,
                 TS = pack_has<ts_source, PER_LCU...> || batch_of<ARGS>::ts, CABAC = pack_has<cabac_source, PER_LCU...>;
  static_assert(!TS || N == 4, "transform skip: 4x4 TUs only");
  static_assert(!CABAC || (TS && !MULTI), "CABAC pricing: the single-picture transform-skip launch only");
  constexpr int TPB = 256 / N, W4 = N / 4;
  constexpr int LD = lds_tile_ld(N);
  __shared__ __attribute__((aligned(16))) i16 sa[TPB * N * LD];     // residual / coefficients
  __shared__ __attribute__((aligned(16))) i16 sb[TPB * N * LD];     // transform scratch
  __shared__ __attribute__((aligned(16))) i16 sq[TPB * N * LD];     // quantized coefficients
  __shared__ int s_has[TPB];

  const auto a = picture_of(args);                                         // the call's picture, or this workgroup's
  if constexpr (MULTI) {
    // launch_size below, per picture; a workgroup beyond its picture's slots leaves with the others that hold no TU
    nx_y = (a.width + N - 1) / N; n_y = nx_y * ((a.height + N - 1) / N);
    nx_c = ((a.width >> 1) + N - 1) / N; n_c = (a.chroma && N < 32) ? nx_c * (((a.height >> 1) + N - 1) / N) : 0;
  }
  const int tid = threadIdx.x, tu = tid / N, row = tid % N;
  const int slot = blockIdx.x * TPB + tu;
  int plane = 0, lx = 0, ly = 0, cu_x = 0, cu_y = 0, leaf = 0;
  bool valid = slot < n_y + 2 * n_c;
  if (slot < n_y) {
    const int ty = slot / nx_y;
    lx = N * (slot - ty * nx_y);
    ly = N * ty;
  } else if (valid) {
    int s = slot - n_y;
    plane = 1;
    if (s >= n_c) { s -= n_c; plane = 2; }
    const int ty = s / nx_c;
    lx = 2 * N * (s - ty * nx_c);
    ly = 2 * N * ty;
  }
  valid = valid && lx < a.width && ly < a.height && inter_cu_at(a, lx, ly, cu_x, cu_y, leaf);
  // chroma TUs are half as wide; with 4x4 luma TUs the chroma of the 8x8 area is one 4x4 TU (transform.c:293-313)
  valid = valid && (plane == 0 ? leaf == N : (N == 4 ? leaf <= 8 : leaf == 2 * N));
  if (!__syncthreads_or(valid)) return;

  quant_consts k = plane ? kc : ky;
  k.qtable = nullptr; k.dqtable = nullptr; k.dq_mode = 0;                  // flat lists only
  [[maybe_unused]] int tu_qp = 0;                                          // TS: state->qp of the TU's LCU
  if constexpr (MULTI) {
    // the array's value clamped as in the per-LCU entry, or the picture's QP as it stands as in the one-QP entry; a slot that is no
    // TU runs the barriers with the constants of QP 0 and reads nothing
    constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5;
    const int qp = valid ? (a.lcu_qp ? clip_lcu_qp(a.lcu_qp[(size_t)(ly >> 6) * a.lcus_x + (lx >> 6)]) : a.qp) : 0;
    if constexpr (SL) k = sl_consts(qp, LOG2, plane, 0, a.slice_is_intra, a.signhide, a.quant, a.dequant);   // no TU: the tables of QP 0, inside the arrays
    else k = flat_consts(qp, LOG2, plane, a.slice_is_intra, a.signhide);
    if constexpr (TS) tu_qp = qp;
  } else if constexpr (LCU_QP) {
    constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5;
    // ky and kc are not used.  A slot that is no TU runs the barriers with the constants of QP 0 and reads nothing
    const lcu_qp_source &q = source_of<lcu_qp_source>(per_lcu...);
    if constexpr (SL) {
      // a slot that is no TU reads the tables of QP 0 of its size and plane: inside the arrays
      const sl_source &t = source_of<sl_source>(per_lcu...);
      const int qp = valid ? clip_lcu_qp(q.lcu_qp ? (int)q.lcu_qp[(size_t)(ly >> 6) * a.lcus_x + (lx >> 6)] : t.qp) : 0;
      k = sl_consts(qp, LOG2, plane, 0, q.slice_is_intra, q.signhide, t.quant, t.dequant);
      if constexpr (TS) tu_qp = qp;
    } else if constexpr (TS) {
      // without an array it is the QP of the one-QP entry, which is not clamped
      const int at = valid ? (int)((size_t)(ly >> 6) * a.lcus_x + (lx >> 6)) : 0;
      const int qp = q.lcu_qp ? (valid ? clip_lcu_qp(q.lcu_qp[at]) : 0) : source_of<ts_source>(per_lcu...).qp;
      k = flat_consts(qp, LOG2, plane, q.slice_is_intra, q.signhide);
      tu_qp = qp;
    } else {
      const int qp = valid ? clip_lcu_qp(q.lcu_qp[(size_t)(ly >> 6) * a.lcus_x + (lx >> 6)]) : 0;
      k = flat_consts(qp, LOG2, plane, q.slice_is_intra, q.signhide);
    }
  }
  const int sh = plane ? 1 : 0, px = lx >> sh, py = ly >> sh;
  const u8 *src_row = (plane == 0 ? a.src_y : (plane == 1 ? a.src_u : a.src_v)) + (size_t)(py + row) * (plane ? a.src_stride_c : a.src_stride_y) + px;
  u8 *rec_row = (plane == 0 ? a.rec_y : (plane == 1 ? a.rec_u : a.rec_v)) + (size_t)(py + row) * (plane ? a.rec_stride_c : a.rec_stride_y) + px;
  i16 *ta = sa + tu * N * LD, *tb = sb + tu * N * LD, *tq = sq + tu * N * LD;

  u32 sw[W4], pw[W4];
#pragma unroll
  for (int j = 0; j < W4; ++j) sw[j] = pw[j] = 0u;
  if (valid) {
    load_row<N>(src_row, sw);
    load_row<N>(rec_row, pw);
  }
  u32 zssd = 0;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    const int d = byte_of(sw, x) - byte_of(pw, x);
    ta[row * LD + x] = (i16)d;
    zssd += (u32)(d * d);
  }
  if (row == 0) s_has[tu] = 0;
  __syncthreads();
  transform_2d_lds<N, 0, LD>(ta, tb, row);
  __syncthreads();
  int any = 0;
  if constexpr (SL) {
    // the thread's row of the table is contiguous: 16-byte loads (the arrays and every table in them are 16-byte aligned)
#pragma unroll
    for (int j = 0; j < W4; ++j) {
      const int4 f4 = *(const int4 *)(k.qtable + row * N + 4 * j);
      const int f[4] = { f4.x, f4.y, f4.z, f4.w };
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = quant_listed(ta[row * LD + 4 * j + i], f[i], k);
        tq[row * LD + 4 * j + i] = (i16)v;
        any |= v;
      }
    }
  } else {
#pragma unroll
    for (int x = 0; x < N; ++x) {
      const int v = quant_one(ta[row * LD + x], k.flat_qc, k);
      tq[row * LD + x] = (i16)v;
      any |= v;
    }
  }
  if (k.signhide) {
    __syncthreads();
    if (row == 0) {
      struct lds_view { i16 *p; int ld, n; __device__ i16 &operator[](int i) const { return p[(i / n) * ld + (i % n)]; } };
      lds_view cv = { ta, LD, N }, qv = { tq, LD, N };
      sign_hide_block(cv, qv, N, 0, k);                                       // diagonal: kvz_get_scan_order of an inter CU
    }
    __syncthreads();
    any = 0;
#pragma unroll
    for (int x = 0; x < N; ++x) any |= tq[row * LD + x];
  }
  if (any) atomicOr(&s_has[tu], 1);
  __syncthreads();
  int has = s_has[tu];
  u32 sab = 0;
  if constexpr (SL) {
#pragma unroll
    for (int j = 0; j < W4; ++j) {
      const int4 d4 = *(const int4 *)(k.dqtable + row * N + 4 * j);
      const int d[4] = { d4.x, d4.y, d4.z, d4.w };
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = tq[row * LD + 4 * j + i];
        sab += (u32)(q < 0 ? -q : q);
        ta[row * LD + 4 * j + i] = (i16)dequant_listed(q, d[i], k);
      }
    }
  } else {
#pragma unroll
    for (int x = 0; x < N; ++x) {
      const int q = tq[row * LD + x];
      sab += (u32)(q < 0 ? -q : q);
      ta[row * LD + x] = (i16)dequant_one(q, row * N + x, k);
    }
  }
  __syncthreads();
  transform_2d_lds<N, 1, LD>(ta, tb, row);
  __syncthreads();
  u32 ssd = zssd;                                    // a TU without coefficients keeps its prediction (quant-generic.c:262-271)
  [[maybe_unused]] u32 keep[W4];                     // TS: the pixels of the trial that stands
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
    if constexpr (TS) {
#pragma unroll
      for (int j = 0; j < W4; ++j) keep[j] = ow[j];
    } else {
      if (valid) store_row<N>(rec_row, ow);
    }
  }
  if constexpr (TS) {
    // ---- the second trial, use_trskip = 1 (transform.c:253-258), in the same threads on the same registers: kvz_transformskip is a
    // shift, so nothing crosses rows but the sign-hiding pass and the sums.  A thread reads and writes its own row of ta / tq since
    // the last barrier; the first trial's row of levels waits in registers.  Chroma slots run it too (the barriers are the
    // workgroup's) and never take it.
    [[maybe_unused]] ts_source of_picture = {};                              // several pictures: from the picture's record
    if constexpr (MULTI) of_picture = { a.lcu_bit_cost, a.tr_skip_out, a.bit_cost, 0 };
    const ts_source &ts = source_of<ts_source>(per_lcu..., of_picture);            // the trailing argument where there is one
    const uint2 q1 = make_uint2(*(const u32 *)(tq + row * LD), *(const u32 *)(tq + row * LD + 2));
    int any2 = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) ta[row * LD + x] = (i16)((byte_of(sw, x) - byte_of(pw, x)) * 32);   // << 5: 15 - 8 - log2 4 (transform.c:151-161)
    if constexpr (SL) {
      const int4 f4 = *(const int4 *)(k.qtable + row * 4);
      const int f[4] = { f4.x, f4.y, f4.z, f4.w };
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int v = quant_listed(ta[row * LD + x], f[x], k);
        tq[row * LD + x] = (i16)v;
        any2 |= v;
      }
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int v = quant_one(ta[row * LD + x], k.flat_qc, k);
        tq[row * LD + x] = (i16)v;
        any2 |= v;
      }
    }
    if (k.signhide) {
      __syncthreads();
      if (row == 0) {
        struct lds_view { i16 *p; int ld, n; __device__ i16 &operator[](int i) const { return p[(i / n) * ld + (i % n)]; } };
        lds_view cv = { ta, LD, 4 }, qv = { tq, LD, 4 };
        sign_hide_block(cv, qv, 4, 0, k);
      }
      __syncthreads();
      any2 = 0;
#pragma unroll
      for (int x = 0; x < 4; ++x) any2 |= tq[row * LD + x];
    }
    const int has2 = group_sum<4>(any2 ? 1u : 0u) ? 1 : 0;                 // the TU's four threads are one quad
    u32 sab2 = 0, ssd2 = zssd, o2 = 0;
    int res[4];
    {
      int d[4] = { 0, 0, 0, 0 };
      if constexpr (SL) {
        const int4 d4 = *(const int4 *)(k.dqtable + row * 4);
        d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int q = tq[row * LD + x];
        sab2 += (u32)(q < 0 ? -q : q);
        int c;
        if constexpr (SL) c = dequant_listed(q, d[x], k);
        else c = dequant_one(q, row * 4 + x, k);
        res[x] = (c + 16) >> 5;                                            // kvz_itransformskip (transform.c:169-181)
      }
    }
    if (has2) {
      ssd2 = 0;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const i16 val = (i16)(res[x] + byte_of(pw, x));
        const int c = val < 0 ? 0 : (val > 255 ? 255 : val);
        const int d = byte_of(sw, x) - c;
        ssd2 += (u32)(d * d);
        o2 |= (u32)c << (8 * x);
      }
    }
    // transform.c:244-266: uint32 costs, the transformed trial wins ties
    u32 bit_cost = 0;
    if (valid) {
      const int v = ts.lcu_bit_cost ? ts.lcu_bit_cost[(size_t)(ly >> 6) * a.lcus_x + (lx >> 6)] : ts.bit_cost;
      bit_cost = (u32)max(v, 0);
    }
    [[maybe_unused]] u32 price1 = 0, price2 = 0;
    if constexpr (CABAC) {
      price1 = trskip_coeff_cost(group_sum<4>(sab), tu_qp);
      price2 = trskip_coeff_cost(group_sum<4>(sab2), tu_qp);
      // rdo.c:214 per TU.  The transformed trial's levels go to the transform scratch, the skipped trial's are in tq; the TU's first
      // thread prices one after the other, each on a fresh copy of its LCU's set, which the TU's four threads make.  Every thread
      // of the workgroup runs the barriers; a slot that is no luma TU, or whose LCU lies below the limit, copies and prices nothing
      __shared__ u8 s_cabac[kvzhip::CC_CTX_USED * TPB];
      const cabac_source &cb = source_of<cabac_source>(per_lcu...);
      const bool on = valid && plane == 0 && tu_qp >= cb.fast_limit;
      const kvz_hip_coeff_ctx *set = cb.sets;
      if (on) {
        const u32 want = cb.lcu_ctx ? (u32)cb.lcu_ctx[(size_t)(ly >> 6) * a.lcus_x + (lx >> 6)] : 0u;
        set += min(want, cb.n_sets - 1u);                                     // an index beyond the table is its last set
      }
      *(u32 *)(tb + row * LD) = q1.x;
      *(u32 *)(tb + row * LD + 2) = q1.y;
      const kvzhip::coeff_cabac_flags fl = { k.signhide != 0, true, false };
      u32 bits[2] = { 0u, 0u };
#pragma unroll
      for (int trial = 0; trial < 2; ++trial) {
        if (on)
          for (int i = row; i < kvzhip::CC_CTX_USED; i += 4) s_cabac[i * TPB + tu] = set->ctx[i];
        __syncthreads();
        if (on && row == 0) {
          const cabac_lds_coeffs cf = { trial ? tq : tb, LD };
          const cabac_lds_ctx<TPB> ctx = { s_cabac + tu };
          bits[trial] = kvzhip::coeff_cabac_count(cf, ctx, set->range, 2, 0, 0, 0u, fl, (trial ? has2 : has) ? 1ull : 0ull);   // inter: diagonal
        }
        __syncthreads();
      }
      const u32 b1 = group_sum<4>(bits[0]), b2 = group_sum<4>(bits[1]);
      if (on) { price1 = b1; price2 = b2; }
    }
    const u32 cost1 = group_sum<4>(ssd) + (CABAC ? price1 : trskip_coeff_cost(group_sum<4>(sab), tu_qp)) * bit_cost;
    const u32 cost2 = group_sum<4>(ssd2) + (CABAC ? price2 : trskip_coeff_cost(group_sum<4>(sab2), tu_qp)) * bit_cost;
    const bool skip = plane == 0 && cost1 > cost2;
    if (skip) {
      has = has2; ssd = ssd2; sab = sab2; keep[0] = o2;
    } else {
      *(u32 *)(tq + row * LD) = q1.x;
      *(u32 *)(tq + row * LD + 2) = q1.y;
    }
    if (valid && has) store_row<N>(rec_row, keep);
    if (valid && plane == 0 && row == 0) ts.tr_skip_out[(size_t)(ly >> 2) * a.cus_stride + (lx >> 2)] = skip ? 1 : 0;
  }
  if (valid) {
    const int bx = (lx & 63) >> (2 + sh), by = (ly & 63) >> (2 + sh);
    const size_t lcu = (size_t)(ly >> 6) * a.lcus_x + (lx >> 6);
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
    ssd = group_sum<N>(ssd);
    zssd = group_sum<N>(zssd);
    sab = group_sum<N>(sab);
    if (valid && row == 0) {
      u32 *c = a.cost + ((size_t)(cu_y >> 2) * a.cus_stride + (cu_x >> 2)) * 6 + sh;
      atomicAdd(c, ssd);
      atomicAdd(c + 2, zssd);
      atomicAdd(c + 4, sab);
    }
  }
}

// the slots of a launch of size N over one picture (the kernel's comment above), and the workgroups that hold them
struct resid_slots { int nx_y, n_y, nx_c, n_c, groups; };
template <int N>
resid_slots residual_slots(int width, int height, int chroma)
{
  resid_slots s;
  s.nx_y = (width + N - 1) / N; s.n_y = s.nx_y * ((height + N - 1) / N);
  s.nx_c = ((width >> 1) + N - 1) / N; s.n_c = (chroma && N < 32) ? s.nx_c * (((height >> 1) + N - 1) / N) : 0;
  constexpr int TPB = 256 / N;
  s.groups = (s.n_y + 2 * s.n_c + TPB - 1) / TPB;
  return s;
}

template <int N, typename... PER_LCU>
void launch_size(const resid_args &a, const quant_consts &ky, const quant_consts &kc, int chroma, hipStream_t st, PER_LCU... q)
{
  const resid_slots n = residual_slots<N>(a.width, a.height, chroma);
  hipLaunchKernelGGL((inter_residual_tu_kernel<N, resid_args, PER_LCU...>), dim3((unsigned)n.groups), dim3(256), 0, st, a, ky, kc, n.nx_y, n.n_y, n.nx_c, n.n_c, q...);
}

// several pictures (BATCH: resid_batch or a resid_batch_ts): workgroups of the launch of size N for the picture with the most slots
template <int N, typename BATCH>
void launch_pictures(const BATCH &b, int n_pictures, hipStream_t st)
{
  int groups = 0;
  for (int i = 0; i < n_pictures; ++i) groups = max(groups, residual_slots<N>(b.p[i].width, b.p[i].height, b.p[i].chroma).groups);
  const quant_consts none = {};                                               // not read: every TU derives its own
  hipLaunchKernelGGL((inter_residual_tu_kernel<N, BATCH>), dim3((unsigned)groups, (unsigned)n_pictures), dim3(256), 0, st, b, none, none, 0, 0, 0, 0);
}

template <typename... PER_LCU>
void launch_width(int n, const resid_args &a, const quant_consts &ky, const quant_consts &kc, int chroma, hipStream_t st, PER_LCU... q)
{
  if (n == 32) launch_size<32>(a, ky, kc, chroma, st, q...);
  else if (n == 16) launch_size<16>(a, ky, kc, chroma, st, q...);
  else if (n == 8) launch_size<8>(a, ky, kc, chroma, st, q...);
  else launch_size<4>(a, ky, kc, chroma, st, q...);
}

// the single-picture entries on their record (chain_picture_pack): p.lcu_qp == nullptr is one QP per call (p.params.qp).  SL: the entry
// with scaling lists, tables required; it launches the kernels that take them and no other, so each translation unit instantiates its
// own kernels only.  TS: the 4x4 launch takes *skip (checked by the caller), and *price with CABAC; the launches of the other sizes
// are those of the entry without it
template <bool SL, bool TS = false, bool CABAC = false>
int residual_frame(const char *entry, const kvz_hip_chain_picture &p, const kvz_hip_scaling_tables *tables, kvz_hip_stream s,
                   const ts_source *skip = nullptr, const cabac_source *price = nullptr)
{
  if (!chain_picture_args_ok(p, false, SL) || (SL && (!tables || !chain_tables_ok(*tables))) || !chain_one_qp_ok(p)) return kvzhip::invalid_arg(entry);
  const int chroma = p.params.chroma ? 1 : 0;
  resid_args a;
  fill(a, p);
  hipStream_t st = ctx_stream(s);
  if (int e = residual_init(a, st)) return e;
  const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
  const lcu_qp_source per_lcu = qp_source_of(p);
  quant_consts ky = {}, kc = {};                                              // read by the kernel without a trailing source only
  for (int n = 32; n >= 4; n >>= 1) {
    if constexpr (SL) {
      const sl_source lists = { tables->quant, tables->dequant, p.params.qp };
      if (!TS || n != 4) launch_width(n, a, ky, kc, chroma, st, per_lcu, lists);
      else if constexpr (CABAC) launch_size<4>(a, ky, kc, chroma, st, per_lcu, lists, *skip, *price);
      else if constexpr (TS) launch_size<4>(a, ky, kc, chroma, st, per_lcu, lists, *skip);
    } else if (TS && n == 4) {
      if constexpr (CABAC) launch_size<4>(a, ky, kc, chroma, st, per_lcu, *skip, *price);
      else if constexpr (TS) launch_size<4>(a, ky, kc, chroma, st, per_lcu, *skip);
    } else if (p.lcu_qp) {
      launch_width(n, a, ky, kc, chroma, st, per_lcu);
    } else {
      // quant uses type 0 / 2, dequant 0 / 2 / 3 (quant-generic.c:224, :244); flat lists: U and V share their constants.  The shift of
      // the transform depends on the size: q_bits, add and the dequantisation shift per launch
      if (!make_consts(&qp, n, 0, 0, &ky) || !make_consts(&qp, n, 2, 2, &kc)) return kvzhip::invalid_arg(entry);
      launch_width(n, a, ky, kc, chroma, st);
    }
    KVZ_CHECK_LAUNCH("inter_residual_tu_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

// intra_recon_core.h -- the kernels and the host side of the whole-picture intra entries (intra_recon.hip: one QP per call,
// intra_recon_qp.hip: a QP per LCU, intra_recon_tiles.hip: a tiled picture, intra_recon_sl.hip: scaling lists, intra_recon_ts.hip:
// transform skip, intra_recon_multi.hip: several pictures in one call, intra_recon_multi_ts.hip: several pictures with tiles, scaling
// lists and transform skip, intra_recon_rdoq.hip: RDOQ, intra_recon_multi_rdoq.hip: several pictures with RDOQ).  Everything here has
// internal linkage: each of the translation units gets its own copy and instantiates exactly one of the kernels.  The algorithm is
// described in intra_recon.hip.
#pragma once

#include "kvz_hip_internal.h"
#include "transform_core.h"
#include "quant_core.h"
#include "lcu_layout.h"
#include "frame_sources.h"
#include "intra_core.h"
#include "tile_grid.h"
#include "coeff_cabac_core.h"

using namespace kvzhip;

namespace {

static_assert(sizeof(kvz_hip_inter_residual_params) == 24 && sizeof(kvz_hip_inter_residual_cost) == 24 && sizeof(kvz_hip_cu_info) == 20,
              "layouts documented in kvz_hip.h");

struct intra_args {
  const u8 *src[3];
  u8 *rec[3];
  u32 src_stride[3], rec_stride[3];
  i16 *coeff[3];
  u32 *cus;                      // records as five dwords; cbf_y is byte 4
  const u8 *modes;               // two bytes per SCU: intra.mode, intra.mode_chroma
  u8 *cbf_out;                   // or nullptr
  u32 *cost;                     // six dwords per SCU, or nullptr
  int cus_stride, lcus_x;
  int width, height;
  quant_consts k[2][4];          // [luma / chroma][log2 N - 2]
};

// One picture of a multi-picture call (kvz_hip_intra_recon_frames): what intra_args holds without the host-made constants, under the
// same member names, and what the workgroup derives its constants from instead (flat_consts with lcu_qp[] or qp, as the per-LCU
// kernel does).  152 bytes; sixteen of them are the kernel's argument, and a workgroup reads its own at blockIdx.z: every address is
// wave-uniform and in the kernel-argument segment, so the fields come through scalar loads into scalar registers.
struct intra_pic {
  const u8 *src[3];
  u8 *rec[3];
  i16 *coeff[3];
  u32 *cus;
  const u8 *modes;
  u8 *cbf_out;                   // or nullptr
  u32 *cost;                     // or nullptr
  const int8_t *lcu_qp;          // or nullptr: qp in every LCU
  u32 src_stride[3], rec_stride[3];
  int qp;
  uint16_t width, height, cus_stride, lcus_x;      // a picture is at most 16384 wide and high
  u8 chroma, slice_is_intra, signhide, pad;
};
struct intra_batch { intra_pic p[KVZ_HIP_MAX_CHAIN_PICTURES]; };
// a checked record into the kernel's; qp: the picture's QP as the kernel is to see it (as it stands, or clamped: the entries differ)
inline void fill(intra_pic &a, const kvz_hip_chain_picture &p, int qp)
{
  const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
  a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.src_stride[0] = p.src.stride_y; a.src_stride[1] = a.src_stride[2] = p.src.stride_c;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = a.rec_stride[2] = p.stride_c;
  a.coeff[0] = p.coeff_y; a.coeff[1] = chroma ? p.coeff_u : nullptr; a.coeff[2] = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.modes = p.intra_modes; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs; a.lcu_qp = p.lcu_qp;
  a.qp = qp;
  a.width = (uint16_t)width; a.height = (uint16_t)height; a.cus_stride = (uint16_t)(width >> 2); a.lcus_x = (uint16_t)((width + 63) >> 6);
  a.chroma = (u8)chroma; a.slice_is_intra = p.params.slice_is_intra ? 1 : 0; a.signhide = p.params.signhide ? 1 : 0;
}
static_assert(sizeof(intra_pic) == 152 && sizeof(intra_batch) <= 3072, "the records travel in the kernel arguments");
template <typename ARGS> struct picture_type { using type = ARGS; };
template <> struct picture_type<intra_batch> { using type = intra_pic; };

// One picture of kvz_hip_intra_recon_frames_ts: intra_pic, then what the _sl and _ts entries take as trailing arguments, and the
// picture's tile grid as counts and offsets into the pool of boundaries that the records of a call share.  cols == 0: no grid, one
// tile.  200 bytes.  Sixteen kvz_hip_tile_grid (392 bytes each) do not fit the kernel arguments beside sixteen records, the
// boundaries that a call uses do: LCU indices are at most 256, two of them to a dword, and the dword is read with a scalar load.
struct intra_pic_ts : intra_pic {
  const int32_t *quant, *dequant;          // SL: the packed tables
  const int32_t *lcu_bit_cost;             // TS: or nullptr, bit_cost in every LCU
  u8 *tr_skip_out;                         // TS
  int bit_cost;
  uint16_t col_at, row_at;                 // where col_bd[0] and row_bd[0] stand in the pool
  u8 cols, rows, pad2[2];
};
struct intra_batch_ts_data {
  intra_pic_ts p[KVZ_HIP_MAX_CHAIN_PICTURES];
  u32 bd[KVZ_HIP_CHAIN_TILE_BOUNDS / 2];
  __device__ __forceinline__ int bound(int i) const { return (int)((bd[i >> 1] >> (16 * (i & 1))) & 0xffffu); }
};
// the options that select an instantiation are the type of the table: a call is homogeneous in them
template <bool SL, bool TS> struct intra_batch_ts : intra_batch_ts_data {};
static_assert(sizeof(intra_pic_ts) == 200 && sizeof(intra_batch_ts_data) == 3200 + 2 * KVZ_HIP_CHAIN_TILE_BOUNDS && sizeof(intra_batch_ts<true, true>) + 8 <= 4096,
              "the records and the pool travel in the kernel arguments: 4 KB with the wave index");
template <bool SL, bool TS> struct picture_type<intra_batch_ts<SL, TS>> { using type = intra_pic_ts; };
// what the type of the kernel's first argument says about the instantiation
template <typename ARGS> struct batch_of { static constexpr bool multi = false, tiles = false, sl = false, ts = false, rdoq = false; };
template <> struct batch_of<intra_batch> { static constexpr bool multi = true, tiles = false, sl = false, ts = false, rdoq = false; };
template <bool SL, bool TS> struct batch_of<intra_batch_ts<SL, TS>> { static constexpr bool multi = true, tiles = true, sl = SL, ts = TS, rdoq = false; };

// One picture of kvz_hip_intra_recon_frames_rdoq: intra_pic, the picture's scaling tables, its own context sets, states and set index
// per LCU, and its tile grid in the pool as in intra_pic_ts.  208 bytes.  The RDOQ tables and rdoq_skip are the call's, once beside
// the records: a pair of pointers per record more would pass the 4 KB of the kernel arguments.
struct intra_pic_rdoq : intra_pic {
  const int32_t *quant, *dequant;          // SL: the packed tables
  const kvz_hip_coeff_ctx *sets;
  const kvz_hip_rdoq_state *states;
  const uint16_t *lcu_ctx;                 // or nullptr: set 0 in every LCU
  u32 n_sets;
  uint16_t col_at, row_at;                 // where col_bd[0] and row_bd[0] stand in the pool
  u8 cols, rows, pad2[6];
};
struct intra_batch_rdoq_data {
  intra_pic_rdoq p[KVZ_HIP_MAX_CHAIN_PICTURES];
  u32 bd[KVZ_HIP_CHAIN_TILE_BOUNDS / 2];
  const int32_t *quant;                    // kvz_hip_rdoq_tables of the call
  const double *err_scale;
  int skip, pad;
  __device__ __forceinline__ int bound(int i) const { return (int)((bd[i >> 1] >> (16 * (i & 1))) & 0xffffu); }
};
template <bool SL> struct intra_batch_rdoq : intra_batch_rdoq_data {};
static_assert(sizeof(intra_pic_rdoq) == 208 && sizeof(intra_batch_rdoq_data) == 3328 + 2 * KVZ_HIP_CHAIN_TILE_BOUNDS + 24 &&
              sizeof(intra_batch_rdoq<true>) + 8 <= 4096, "the records, the pool and the shared tables travel in the kernel arguments: 4 KB with the wave index");
template <bool SL> struct picture_type<intra_batch_rdoq<SL>> { using type = intra_pic_rdoq; };
template <bool SL> struct batch_of<intra_batch_rdoq<SL>> { static constexpr bool multi = true, tiles = true, sl = SL, ts = false, rdoq = true; };

// The LCU's tile in LDS: pixel (x, y) of the plane relative to the LCU's top-left, x = -1 .. T + T/2 - 1, y = -1 .. T - 1
// (T = 64 luma, 32 chroma).  Column 0 stands at a dword boundary.
constexpr int TS = 104, TILE_BYTES = 65 * TS;
__device__ __forceinline__ int tpx(int x, int y) { return (y + 1) * TS + 4 + x; }

// the intra CU that holds the luma position (x, y), from the record of that position alone: false for another type, a
// depth beyond 3 or a CU that would leave the picture (the rule of kvz_hip_inter_residual_frame with the type swapped)
__device__ __forceinline__ bool intra_cu_of(u32 head, int x, int y, int width, int height, int &cu_x, int &cu_y, int &leaf)
{
  const int depth = (head >> 8) & 255, trd = (int)(head >> 24);
  if ((head & 255u) != 1u || depth > 3) return false;                         // CU_INTRA (cu.h:38-43)
  const int size = 64 >> depth;
  cu_x = x & ~(size - 1);
  cu_y = y & ~(size - 1);
  leaf = 64 >> min(4, max(max(depth, trd), 1));
  return cu_x + size <= width && cu_y + size <= height;
}

// the rule as the init kernels ask it (zero_cu_outputs, frame_sources.h): SCU i of picture a, which lies at luma (x, y)
struct intra_cu_rule {
  template <typename PIC> __device__ __forceinline__ bool operator()(const PIC &a, int i, int x, int y, int &cu_x, int &cu_y, int &leaf) const
  {
    return intra_cu_of(a.cus[(size_t)i * 5], x, y, a.width, a.height, cu_x, cu_y, leaf);
  }
};

// cbf_out and costs start from zero inside the intra CUs
__global__ __launch_bounds__(256) void intra_recon_init_kernel(intra_args a, int n_scu)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_scu) return;
  zero_cu_outputs(a, i, intra_cu_rule());
}

struct tu_pos {
  int plane, sh;                 // sh = 1 for chroma
  int lx, ly;                    // luma position in the picture
  int tx, ty;                    // position in the tile, in pixels of the plane
  int cu_x, cu_y;
  int mode, scan;
};

// the rectangle a TU takes its neighbours from, in luma pixels: the picture, or the TU's tile (state->tile->frame of the reference)
struct tile_rect { int x0, y0, x1, y1; };

struct lds_view { i16 *p; int ld, n; __device__ i16 &operator[](int i) const { return p[(i / n) * ld + (i % n)]; } };

// what a 4x4 luma TU needs for the two trials of transform skip: state->qp and the bit cost of its LCU, and where the choice goes
struct ts_lcu { int qp; u32 bit_cost; u8 *out; };
// CABAC pricing of the two trials: the LCU's context set, and whether its QP is at or above cfg.fast_residual_cost_limit (rdo.c:214)
struct cabac_lcu { const kvz_hip_coeff_ctx *set; bool on; };
struct cabac_lds_ctx {
  u8 *p;
  __device__ __forceinline__ u32 get(int i) const { return p[i]; }
  __device__ __forceinline__ void set(int i, u32 v) { p[i] = (u8)v; }
};

// One leaf TU, N wide, by the whole wave.  Called under wave-uniform conditions only.  TILES: tr stands for the picture in everything
// about the TU's neighbours; without it tr is not read, and the code is compiled from the expressions it always had.  SL: k carries the
// TU's tables (sl_consts, quant_core.h); a lane reads its row of each, which is contiguous, with 16-byte loads.
// TS (N = 4): a luma TU is coded twice side by side, transformed on lanes 0-3 and transform-skipped on lanes 4-7, which repeat rows
// 0-3 on a second set of LDS rows (kvz_quantize_residual_trskip, transform.c:229-276).  Both trials share the prediction and run every
// step in the same instructions; the skipped one replaces the transforms' results by the shifts of kvz_transformskip /
// kvz_itransformskip.  They meet once, after the reconstruction: each quad sums its SSD and |coeff|, prices its trial, reads the
// other quad's cost through a lane exchange, and the lanes of the trial that stands write the tile, the coefficients and the flags.
// The lanes beyond 8 repeat lane % 8.  A chroma TU of the same kernel is coded as without TS.
// CABAC (with TS): where the LCU's QP is at or above the limit, a trial's price is get_coeff_cabac_cost of its 16 levels
// (coeff_cabac_core.h) instead of the estimate: the first lane of each trial's quad counts on a copy of the LCU's set of its own.
// RQ (rdoq_lcu<true>, rdoq_stage.h; without TS): a TU that takes RDOQ gets its levels from kvz_rdoq on the coefficient rows instead of
// the quantiser and its sign hiding; tr_depth is what kvz_quantize_residual hands over for the TU.  Everything after the levels is shared.
template <int N, bool TILES, bool SL = false, bool TS = false, bool CABAC = false, typename ARGS, typename RQ = rdoq_lcu<false>>
__device__ __forceinline__ void intra_tu(const ARGS &a, const tu_pos &t, const tile_rect &tr, const quant_consts &k, u8 *tile, u8 (*s_ref)[RS],
                                        u8 *s_ext, u8 *s_pred, i16 *ta, i16 *tb, i16 *tq, const ts_lcu ts = {}, const cabac_lcu cb = {},
                                        const RQ rq = {}, int tr_depth = 0)
{
  static_assert(!RQ::on || !TS, "RDOQ: not together with transform skip");
  static_assert(!TS || N == 4, "transform skip: 4x4 TUs only");
  static_assert(!CABAC || TS, "CABAC pricing belongs to the transform-skip decision");
  constexpr int LOG2 = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5, LD = lds_tile_ld(N), W4 = N / 4;
  const int lane = threadIdx.x, row = lane & (N - 1);
  bool own = lane < N;                                           // the lanes that touch global memory
  const int sh = t.sh, flags = t.plane == 0 ? (KVZ_HIP_INTRA_LUMA | KVZ_HIP_INTRA_FILTER_BOUNDARY) : 0;

  // ---- kvz_intra_build_reference (intra.c:334-588) from the tile, as intra_build_reference_kernel takes it from the plane ----
  for (int i = lane; i < 4 * RS / 4; i += 64) ((u32 *)s_ref)[i] = 0u;
  __syncthreads();
  if (lane < 2 * N) {
    const int ux = (t.lx & 63) >> 2, uy = (t.ly & 63) >> 2;
    bool has_left = t.lx > 0, has_top = t.ly > 0;
    if constexpr (TILES) { has_left = t.lx > tr.x0; has_top = t.ly > tr.y0; }
    u8 left, top;
    if (has_left) {
      int avail = intra_coded_left(ux, uy) >> sh;
      if constexpr (TILES) avail = min(avail, min(2 * N, (tr.y1 - t.ly) >> sh));
      else avail = min(avail, min(2 * N, (a.height - t.ly) >> sh));
      left = tile[tpx(t.tx - 1, t.ty + min(lane, avail - 1))];
    } else {
      left = has_top ? tile[tpx(t.tx, t.ty - 1)] : 128;
    }
    if (has_top) {
      int avail = intra_coded_above(ux, uy) >> sh;
      if constexpr (TILES) avail = min(avail, min(2 * N, (tr.x1 - t.lx) >> sh));
      else avail = min(avail, min(2 * N, (a.width - t.lx) >> sh));
      top = tile[tpx(t.tx + min(lane, avail - 1), t.ty - 1)];
    } else {
      top = has_left ? tile[tpx(t.tx - 1, t.ty)] : 128;
    }
    s_ref[0][1 + lane] = left;
    s_ref[1][1 + lane] = top;
    if (lane == 0) {
      const u8 corner = (has_left && has_top) ? tile[tpx(t.tx - 1, t.ty - 1)] : (has_left ? tile[tpx(t.tx - 1, t.ty)] : left);
      s_ref[0][0] = corner;
      s_ref[1][0] = corner;
    }
  }
  __syncthreads();
  // smoothed references (intra.c:164-192)
  for (int i = lane; i < 2 * (2 * N + 1); i += 64) {
    const int s = i >= 2 * N + 1, e = i - (2 * N + 1) * s;
    const u8 *from = s_ref[s];
    int v;
    if (e == 0) v = (s_ref[0][1] + 2 * s_ref[0][0] + s_ref[1][1] + 2) >> 2;
    else if (e == 2 * N) v = from[e];
    else v = (from[e - 1] + 2 * from[e] + from[e + 1] + 2) >> 2;
    s_ref[2 + s][e] = (u8)v;
  }
  __syncthreads();

  // ---- kvz_intra_predict (intra.c:281-331) ----
  const bool fil = use_filtered(t.mode, LOG2, flags), edge = luma_edge_filters(LOG2, flags);
  if (t.mode >= 2) {
    const ang_t an = ang_of(t.mode);
    for (int e = lane; e < 3 * N + 2; e += 64) s_ext[e] = ext_entry<N>(s_ref, fil, an, e - N);
    __syncthreads();
    const u8 *e = &s_ext[N];
    const u8 *side = s_ref[2 * fil + (an.vertical ? 0 : 1)];
    const bool pp = edge && (flags & KVZ_HIP_INTRA_FILTER_BOUNDARY) && an.disp == 0;
    for (int px = lane; px < N * N; px += 64) {
      const int y = px >> LOG2, x = px & (N - 1);
      const int r = an.vertical ? y : x, c = an.vertical ? x : y;
      int v = ang_px(e, an.disp, r, c);
      if (pp && c == 0) v = post_px(v, side, r);
      s_pred[px] = (u8)v;
    }
  } else if (t.mode == 1) {
    const int dc = dc_value(s_ref, N, LOG2);
    for (int px = lane; px < N * N; px += 64) s_pred[px] = (u8)dc_px(s_ref, dc, edge, px & (N - 1), px >> LOG2);
  } else {
    const u8 *left = s_ref[2 * fil], *top = s_ref[2 * fil + 1];
    for (int px = lane; px < N * N; px += 64) s_pred[px] = (u8)planar_px(left, top, N, LOG2, px & (N - 1), px >> LOG2);
  }
  __syncthreads();

  // ---- kvz_quantize_residual (quant-generic.c:180-273), the arithmetic of inter_residual_tu_kernel ----
  const int px0 = t.lx >> sh, py0 = t.ly >> sh;
  u32 sw[W4], pw[W4];
  load_row<N>(a.src[t.plane] + (size_t)(py0 + row) * a.src_stride[t.plane] + px0, sw);      // lanes beyond N: the row of lane % N again
#pragma unroll
  for (int j = 0; j < W4; ++j) pw[j] = *(const u32 *)(s_pred + row * N + 4 * j);
  [[maybe_unused]] bool dual = false;                                           // TS: a luma TU, two trials (wave-uniform)
  [[maybe_unused]] int trial = 0;                                               // TS: 0 transformed, 1 skipped
  if constexpr (TS) {
    dual = t.plane == 0;
    trial = dual ? (lane >> 2) & 1 : 0;
    ta += trial * 4 * LD; tb += trial * 4 * LD; tq += trial * 4 * LD;          // each trial on LDS rows of its own
  }
  u32 zssd = 0;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    const int d = byte_of(sw, x) - byte_of(pw, x);
    ta[row * LD + x] = (i16)d;
    zssd += (u32)(d * d);
  }
  __syncthreads();
  if constexpr (N == 4) {
    if (t.plane == 0) transform_2d_lds<4, 2, LD>(ta, tb, row);                // strategies-dct.c:66-85: DST for intra 4x4 luma
    else transform_2d_lds<4, 0, LD>(ta, tb, row);
  } else {
    transform_2d_lds<N, 0, LD>(ta, tb, row);
  }
  __syncthreads();
  if constexpr (TS) {
    // kvz_transformskip (transform.c:151-161): << 15 - 8 - log2 4.  The skipped trial ran the transform above with the other one, on
    // its own rows, and drops the result
    if (trial) {
#pragma unroll
      for (int x = 0; x < 4; ++x) ta[row * LD + x] = (i16)((byte_of(sw, x) - byte_of(pw, x)) * 32);
    }
  }
  int any = 0;
  [[maybe_unused]] bool rdoq = false;                                           // RQ: kvz_rdoq instead of kvz_quant (wave-uniform)
  if constexpr (RQ::on) {
    rdoq = rq.takes(N);
    if (rdoq) {
      rq.template tu<N, LD>(ta, tq, lane, t.plane ? 2 : 0, t.scan, 1, tr_depth);
#pragma unroll
      for (int x = 0; x < N; ++x) any |= tq[row * LD + x];
    }
  }
  if (rdoq) {
    // the levels are kvz_rdoq's, its own sign hiding included
  } else if constexpr (SL) {
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
  if (k.signhide && !rdoq) {
    // a lane per coefficient group, as sign_hide_kernel (quant.hip): the block's ac_sum is a sum over the lanes, the "last"
    // group a ballot of the lanes that hold a level
    __syncthreads();
    constexpr int NCG = W4 * W4;
    const lds_view cv = { ta, LD, N }, qv = { tq, LD, N };
    int pos16[16];
    bool nz = false;
    u32 ac = 0;
    if constexpr (TS) {
      // one coefficient group per trial, on the trial's first lane: its ac_sum is the lane's own, and it is the last group if it
      // holds a level
#pragma unroll
      for (int n = 0; n < 16; ++n) {
        pos16[n] = scan_pos(t.scan, 2, n);
        nz = nz || qv[pos16[n]] != 0;
        if constexpr (SL) ac += (u32)quant_level(cv[pos16[n]], k.qtable[pos16[n]], k);
        else ac += (u32)quant_level(cv[pos16[n]], k.flat_qc, k);
      }
      if (lane == 4 * trial && ac >= 2) sign_hide_cg(cv, qv, pos16, nz, k);
    } else {
      const bool cg_ok = lane < NCG;
#pragma unroll
      for (int n = 0; n < 16; ++n) {
        pos16[n] = scan_pos(t.scan, LOG2, ((cg_ok ? lane : 0) << 4) + n);
        nz = nz || qv[pos16[n]] != 0;
        if constexpr (SL) ac += (u32)quant_level(cv[pos16[n]], k.qtable[pos16[n]], k);
        else ac += (u32)quant_level(cv[pos16[n]], k.flat_qc, k);
      }
      ac = group_sum<64>(cg_ok ? ac : 0u);
      const unsigned long long bal = __ballot(nz && cg_ok);
      const bool is_last = nz && (bal & ~((2ull << lane) - 1ull)) == 0ull;
      if (cg_ok && ac >= 2) sign_hide_cg(cv, qv, pos16, is_last, k);
    }
    __syncthreads();
    any = 0;
#pragma unroll
    for (int x = 0; x < N; ++x) any |= tq[row * LD + x];
  }
  int has;
  if constexpr (TS) {
    // has_coeffs of the lane's own trial: lanes 0-3 and 4-7 hold the rows of the two trials (of the one trial for a chroma TU)
    const unsigned long long bal = __ballot(any != 0);
    __syncthreads();
    has = ((bal >> (4 * trial)) & 15ull) ? 1 : 0;
  } else {
    has = __syncthreads_or(any) ? 1 : 0;
  }
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
  [[maybe_unused]] int skipped[4];                                              // TS: kvz_itransformskip (transform.c:169-181) of the lane's row
  if constexpr (TS) {
#pragma unroll
    for (int x = 0; x < 4; ++x) skipped[x] = ((int)ta[row * LD + x] + 16) >> 5;
  }
  __syncthreads();
  if constexpr (N == 4) {
    if (t.plane == 0) transform_2d_lds<4, 3, LD>(ta, tb, row);
    else transform_2d_lds<4, 1, LD>(ta, tb, row);
  } else {
    transform_2d_lds<N, 1, LD>(ta, tb, row);
  }
  __syncthreads();
  // the reconstruction goes into the tile; a TU without coefficients keeps its prediction (quant-generic.c:262-271)
  u32 ssd = zssd;
  if (has) ssd = 0;
  [[maybe_unused]] u32 kept = 0;                                                // TS: the lane's row of its trial's reconstruction
#pragma unroll
  for (int j = 0; j < W4; ++j) {
    u32 o = pw[j];
    if (has) {
      o = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = 4 * j + i;
        int res = (int)ta[row * LD + x];
        if constexpr (TS) res = trial ? skipped[x] : res;
        const i16 val = (i16)(res + byte_of(pw, x));                               // quant-generic.c:255
        const int c = val < 0 ? 0 : (val > 255 ? 255 : val);
        const int d = byte_of(sw, x) - c;
        ssd += (u32)(d * d);
        o |= (u32)c << (8 * i);
      }
    }
    if constexpr (TS) kept = o;
    else *(u32 *)(tile + tpx(t.tx + 4 * j, t.ty + row)) = o;                    // tx is a multiple of 4: an aligned dword
  }
  if constexpr (TS) {
    // transform.c:244-266: uint32 costs, the transformed trial wins ties.  The lanes of the trial that stands go on as the TU's lanes
    bool stands = true;
    if (dual) {
      [[maybe_unused]] u32 price = 0;
      if constexpr (CABAC) {
        price = trskip_coeff_cost(group_sum<4>(sab), ts.qp);
        if (cb.on) {                                                           // wave-uniform, as dual is
          __shared__ u8 s_cabac[2][kvzhip::CC_CTX_USED + 2];
          for (int i = lane; i < kvzhip::CC_CTX_USED; i += 64) {
            const u8 v = cb.set->ctx[i];
            s_cabac[0][i] = v;
            s_cabac[1][i] = v;
          }
          __syncthreads();
          u32 bits = 0;
          if (lane < 8 && (lane & 3) == 0) {
            const cabac_lds_coeffs cf = { tq, LD };                            // tq is the lane's own trial's rows
            const cabac_lds_ctx ctx = { s_cabac[trial] };
            const kvzhip::coeff_cabac_flags fl = { k.signhide != 0, true, false };
            bits = kvzhip::coeff_cabac_count(cf, ctx, cb.set->range, 2, 0, t.scan, 0u, fl, has ? 1ull : 0ull);
          }
          price = (u32)__shfl((int)bits, lane & 4, 64);                        // the lanes beyond 8 repeat lane % 8
          __syncthreads();
        }
      }
      const u32 cost = group_sum<4>(ssd) + (CABAC ? price : trskip_coeff_cost(group_sum<4>(sab), ts.qp)) * ts.bit_cost;
      const u32 other = (u32)__shfl_xor((int)cost, 4, 64);
      stands = trial ? cost < other : cost <= other;
    }
    if (stands) *(u32 *)(tile + tpx(t.tx, t.ty + row)) = kept;
    own = lane < (dual ? 8 : 4) && stands;
  }
  if (own) {
    const int bx = (t.lx & 63) >> (2 + sh), by = (t.ly & 63) >> (2 + sh);
    const size_t lcu = (size_t)(t.ly >> 6) * a.lcus_x + (t.lx >> 6);
    i16 *dst = a.coeff[t.plane] + lcu * (t.plane ? 1024 : 4096) + 16 * zorder_blk(bx, by) + row * N;
    if (N == 4) {
      *(uint2 *)dst = make_uint2(*(const u32 *)(tq + row * LD), *(const u32 *)(tq + row * LD + 2));
    } else {
#pragma unroll
      for (int j = 0; j < N / 8; ++j) *(uint4 *)(dst + 8 * j) = lds_tile_load8<N, LD>(tq, row * N + 8 * j);
    }
    // flags of the SCUs the TU covers: cbf_y as lcu_set_coeff leaves it (search.c:173-190), bit `plane` of cbf_out (zeroed by
    // the init kernel)
    const int sx0 = t.lx >> 2, sy0 = t.ly >> 2;
    if (t.plane == 0) {
      if ((row & 3) == 0) {
        for (int i = 0; i < W4; ++i) {
          const size_t scu = (size_t)(sy0 + (row >> 2)) * a.cus_stride + sx0 + i;
          ((u8 *)a.cus)[scu * 20 + 4] = (u8)has;
          if (a.cbf_out && has) or_byte(a.cbf_out, scu, 1u);
          if constexpr (TS) ts.out[scu] = (u8)trial;                                 // cur_pu->tr_skip (transform.c:387)
        }
      }
    } else if (row < N / 2 && a.cbf_out && has) {
      for (int i = 0; i < N / 2; ++i) or_byte(a.cbf_out, (size_t)(sy0 + row) * a.cus_stride + sx0 + i, 1u << t.plane);
    }
  }
  if (a.cost) {
    // integer sums: the order of the additions does not matter
    ssd = group_sum<64>(own ? ssd : 0u);
    zssd = group_sum<64>(own ? zssd : 0u);
    sab = group_sum<64>(own ? sab : 0u);
    if (lane == 0) {
      u32 *c = a.cost + ((size_t)(t.cu_y >> 2) * a.cus_stride + (t.cu_x >> 2)) * 6 + sh;
      atomicAdd(c, ssd);
      atomicAdd(c + 2, zssd);
      atomicAdd(c + 4, sab);
    }
  }
  __syncthreads();                                                              // the tile is complete for the next TU
}

// The trailing sources of the kernel below (frame_sources.h), in their order.  Each of them selects an instantiation that is alone in
// its translation unit: a second one in the same module changes the code the compiler emits for the first, and the kernels that were
// there before an option are to stay as they were measured.
// A QP per LCU (kvz_hip_intra_recon_frame_qp, intra_recon_qp.hip) is lcu_qp_source.  A workgroup is one LCU of one plane, so the QP is
// one value per workgroup: loaded once, made wave-uniform, and the sets of the four sizes derived before the walk; they stay in scalar
// registers.  Without it (intra_recon.hip) the sets come in intra_args.
// A tiled picture (kvz_hip_intra_recon_frame_tiles, intra_recon_tiles.hip) is a second trailing argument after the QP source: the
// grid, and the QP of every LCU where the source's array is NULL.
struct tile_source { kvz_hip_tile_grid grid; int qp; };
// Scaling lists (kvz_hip_intra_recon_frame_sl, intra_recon_sl.hip) are a third trailing argument after the grid: the two packed arrays.
// The workgroup derives the sets of the four sizes of its LCU and plane with their table pointers (sl_consts, quant_core.h) where the
// others derive the flat sets.
struct sl_source { const int32_t *quant, *dequant; };
// Transform skip (kvz_hip_intra_recon_frame_ts, intra_recon_ts.hip) comes after the grid or after the lists: the bit cost, one value or
// one per LCU, and the array of choices.  The workgroup reads its LCU's value once, next to the QP.  Two instantiations, flat lists and
// tables.
struct ts_source { const int32_t *lcu_bit_cost; u8 *tr_skip_out; int bit_cost; };
// CABAC pricing of the two trials (kvz_hip_intra_recon_frame_ts_cabac, intra_recon_ts_cabac.hip) is cabac_source, after the
// transform-skip source.  The workgroup picks its LCU's set once, next to the QP.  Two instantiations again.
template <bool LCU_QP> struct lcu_sets {};                                   // what a workgroup derives from its LCU's QP: nothing with one QP per call,
template <> struct lcu_sets<true> { quant_consts k[4]; };                    // else the sets of the four sizes, [log2 N - 2]

// z-order index -> coordinate: the even bits of i
__device__ __forceinline__ int compact4(int i) { i &= 0x55; i = (i | (i >> 1)) & 0x33; return (i | (i >> 2)) & 0x0f; }

// wave t of the picture: grid (lcus_y, planes), LCU (t - 2 ly, ly).  Tiled: grid (lcus_y * cols, planes), a workgroup per LCU row and
// tile column, LCU (x0 + t - 2 (ly - y0), ly) of the tile that begins at LCU (x0, y0): the waves of all tiles share the launches, and the
// rectangle that stands for the picture in everything about neighbours is the tile.  Several pictures (ARGS = intra_batch,
// kvz_hip_intra_recon_frames): grid (max lcus_y, planes, pictures); the workgroup takes its picture's record at blockIdx.z, leaves at
// once where that picture has no such plane, row or wave, and derives its constants as the per-LCU kernel does.  With RDOQ
// (ARGS = intra_batch_rdoq<SL>, kvz_hip_intra_recon_frames_rdoq) it also makes its rdoq_source of its picture's record and the call's
// tables.  WG = 64 is part of the algorithm, not a tuning value: intra_tu lets
// the lanes beyond a TU's N rows repeat row lane % N, which is the same value to the same LDS address only while all of them are
// one wave in lockstep; with a second wave the read-modify-write of ta / tq would race.
constexpr int WG = 64;
static_assert(WG == 64, "one wave per workgroup: see intra_tu");
template <typename ARGS, typename... PER_LCU>
__global__ __launch_bounds__(WG) void intra_recon_wave_kernel(ARGS args, int t, PER_LCU... per_lcu)
{
  constexpr bool MULTI = batch_of<ARGS>::multi, LCU_QP = MULTI || sizeof...(PER_LCU) != 0, TILES = sizeof...(PER_LCU) >= 2 || batch_of<ARGS>::tiles,
                 SL = pack_has<sl_source, PER_LCU...> || batch_of<ARGS>::sl, TS = pack_has<ts_source, PER_LCU...> || batch_of<ARGS>::ts,
                 CABAC = pack_has<cabac_source, PER_LCU...>, RDOQ = pack_has<rdoq_source, PER_LCU...> || batch_of<ARGS>::rdoq;
  static_assert(!RDOQ || (LCU_QP && !TS), "RDOQ: not together with transform skip");
  __shared__ __attribute__((aligned(16))) u8 tile[TILE_BYTES];
  __shared__ __attribute__((aligned(16))) u8 s_ref[4][RS];
  __shared__ __attribute__((aligned(16))) u8 s_ext[3 * 32 + 4];
  __shared__ __attribute__((aligned(16))) u8 s_pred[32 * 32];
  __shared__ __attribute__((aligned(16))) i16 sa[32 * lds_tile_ld(32)];     // residual / coefficients
  __shared__ __attribute__((aligned(16))) i16 sb[32 * lds_tile_ld(32)];     // transform scratch
  __shared__ __attribute__((aligned(16))) i16 sq[32 * lds_tile_ld(32)];     // quantized coefficients
  __shared__ u8 s_intra[256];                                                // SCU (raster) belongs to an intra CU of this call

  // the call's picture, or this workgroup's: picture blockIdx.z of the table.  Bound without a call in between: through a function the
  // one-QP kernel is no longer compiled to the code it was (tools/compare_kernels.py)
  using PIC = typename picture_type<ARGS>::type;
  const PIC &a = ((const PIC *)&args)[MULTI ? blockIdx.z : 0];
  const int lane = threadIdx.x, plane = blockIdx.y, sh = plane ? 1 : 0;
  int lcu_y = blockIdx.x, lcu_x = t - 2 * lcu_y;
  if constexpr (MULTI && !TILES) {
    // the grid is that of the tallest picture with chroma (a wave of a picture that has run out fails the test of lcu_x below)
    if ((plane && !a.chroma) || 64 * lcu_y >= a.height) return;
  }
  tile_rect tr;                                                              // read with tiles only
  if constexpr (MULTI && TILES) {
    // the grid's x extent is that of the picture with the most LCU rows x tile columns.  Wave-uniform: the picture's counts and
    // offsets from its record, its boundaries from the pool, all scalar loads from the kernel arguments
    if (plane && !a.chroma) return;
    const int lcus_y = (a.height + 63) >> 6;
    int cx0 = 0, cx1 = a.lcus_x, ry0 = 0, ry1 = lcus_y;
    if (a.cols) {
      const int cols = a.cols, col = (int)blockIdx.x % cols;
      lcu_y = (int)blockIdx.x / cols;
      if (lcu_y >= lcus_y) return;
      cx0 = args.bound(a.col_at + col);
      cx1 = args.bound(a.col_at + col + 1);
      // row_bd[rows] is the picture's count of LCU rows, above lcu_y: the walk ends at the tile row that holds lcu_y
      for (int j = 1; j <= a.rows; ++j) {
        const int b = args.bound(a.row_at + j);
        if (b > lcu_y) { ry1 = b; break; }
        ry0 = b;
      }
    }
    if (lcu_y >= lcus_y) return;
    lcu_x = cx0 + t - 2 * (lcu_y - ry0);
    if (lcu_x < cx0 || lcu_x >= cx1) return;
    tr = { 64 * cx0, 64 * ry0, min(64 * cx1, (int)a.width), min(64 * ry1, (int)a.height) };
  } else if constexpr (TILES) {
    // wave-uniform: scalar loads of the grid, scalar compares and selects
    const kvz_hip_tile_grid &g = source_of<tile_source>(per_lcu...).grid;
    const int cols = g.cols, col = (int)blockIdx.x % cols;
    int cx0, cx1, ry0, ry1;
    lcu_y = (int)blockIdx.x / cols;
    tile_span_at(g.col_bd, col, cx0, cx1);
    tile_span_of(g.row_bd, g.rows, lcu_y, ry0, ry1);
    lcu_x = cx0 + t - 2 * (lcu_y - ry0);
    if (lcu_x < cx0 || lcu_x >= cx1) return;
    tr = { 64 * cx0, 64 * ry0, min(64 * cx1, a.width), min(64 * ry1, a.height) };
  } else {
    if (lcu_x < 0 || lcu_x >= a.lcus_x) return;
  }
  const int X0 = 64 * lcu_x, Y0 = 64 * lcu_y;

  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j, x = X0 + 4 * (i & 15), y = Y0 + 4 * (i >> 4);
    int cu_x, cu_y, leaf;
    const bool in = x < a.width && y < a.height &&
                    intra_cu_of(a.cus[((size_t)(y >> 2) * a.cus_stride + (x >> 2)) * 5], x, y, a.width, a.height, cu_x, cu_y, leaf);
    s_intra[i] = in;
    any = any || in;
  }
  if (!__syncthreads_or(any)) return;

  // ---- the tile: rows -1 .. th - 1 as dwords (the plane's width and the tile's extent are multiples of 4), then the column left ----
  // nothing outside the rectangle is read: with tiles the LCUs beyond it are being written by other workgroups of this launch
  const int T = 64 >> sh;
  int pw = a.width >> sh, ph = a.height >> sh, qx = 0, qy = 0;
  const int x0 = X0 >> sh, y0 = Y0 >> sh;
  if constexpr (TILES) { pw = tr.x1 >> sh; ph = tr.y1 >> sh; qx = tr.x0 >> sh; qy = tr.y0 >> sh; }
  const int tw = min(T, pw - x0), th = min(T, ph - y0), aw = y0 > qy ? min(T + T / 2, pw - x0) : 0;
  u8 *rec = a.rec[plane];
  const size_t stride = a.rec_stride[plane];
  constexpr int CW = (64 + 32) / 4;
  for (int it = lane; it < (th + 1) * CW; it += 64) {
    const int r = it / CW - 1, c4 = 4 * (it % CW);
    if (c4 < (r < 0 ? aw : tw)) {
      u32 v;
      __builtin_memcpy(&v, rec + (size_t)(y0 + r) * stride + x0 + c4, 4);
      *(u32 *)(tile + tpx(c4, r)) = v;
    }
  }
  if (x0 > qx)
    for (int r = lane - 1; r < th; r += 64)
      if (r >= 0 || y0 > qy) tile[tpx(-1, r)] = rec[(size_t)(y0 + r) * stride + x0 - 1];
  __syncthreads();

  lcu_sets<LCU_QP> own;                                                      // the LCU's own sets, [log2 N - 2]
  [[maybe_unused]] ts_lcu skip = {};
  [[maybe_unused]] cabac_lcu price = {};
  [[maybe_unused]] rdoq_lcu<RDOQ> rq = {};
  if constexpr (MULTI) {
    // the array's value clamped as in the per-LCU entry, or the picture's QP as it stands as in the one-QP entry
    const int qp = (int)__builtin_amdgcn_readfirstlane((u32)(a.lcu_qp ? clip_lcu_qp((int)a.lcu_qp[(size_t)lcu_y * a.lcus_x + lcu_x]) : a.qp));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (SL) own.k[i] = sl_consts(qp, 2 + i, plane, 1, a.slice_is_intra, a.signhide, a.quant, a.dequant);
      else own.k[i] = flat_consts(qp, 2 + i, plane ? 1 : 0, a.slice_is_intra, a.signhide);
    }
    if constexpr (TS) {
      const int v = (int)__builtin_amdgcn_readfirstlane((u32)(a.lcu_bit_cost ? a.lcu_bit_cost[(size_t)lcu_y * a.lcus_x + lcu_x] : a.bit_cost));
      skip = { qp, (u32)max(v, 0), a.tr_skip_out };
    }
    if constexpr (RDOQ) {
      // the wave's source from its picture's record and the call's tables (scalar loads from the kernel arguments), then as below
      __shared__ typename rdoq_lcu<RDOQ>::lds s_rdoq;
      rq.m = &s_rdoq;
      rq.r = { a.sets, a.states, a.lcu_ctx, args.quant, args.err_scale, a.n_sets, args.skip };
      rq.qp = qp;
      rq.signhide = a.signhide != 0;
      rq.stage((size_t)lcu_y * a.lcus_x + lcu_x, lane);
    }
  } else if constexpr (LCU_QP) {
    const lcu_qp_source &q = source_of<lcu_qp_source>(per_lcu...);
    int qp;
    if constexpr (TILES) qp = clip_lcu_qp((int)__builtin_amdgcn_readfirstlane((u32)(q.lcu_qp ? (int)q.lcu_qp[(size_t)lcu_y * a.lcus_x + lcu_x] : source_of<tile_source>(per_lcu...).qp)));
    else qp = clip_lcu_qp((int)__builtin_amdgcn_readfirstlane((u32)(int)q.lcu_qp[(size_t)lcu_y * a.lcus_x + lcu_x]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (a chroma plane has no 32x32 TU: that set is derived and not used)
      if constexpr (SL) {
        const sl_source &lists = source_of<sl_source>(per_lcu...);
        own.k[i] = sl_consts(qp, 2 + i, plane, 1, q.slice_is_intra, q.signhide, lists.quant, lists.dequant);
      } else {
        own.k[i] = flat_consts(qp, 2 + i, plane ? 1 : 0, q.slice_is_intra, q.signhide);
      }
    }
    if constexpr (TS) {
      const ts_source &ts = source_of<ts_source>(per_lcu...);
      const int v = (int)__builtin_amdgcn_readfirstlane((u32)(ts.lcu_bit_cost ? ts.lcu_bit_cost[(size_t)lcu_y * a.lcus_x + lcu_x] : ts.bit_cost));
      skip = { qp, (u32)max(v, 0), ts.tr_skip_out };
    }
    if constexpr (CABAC) {
      const cabac_source &cb = source_of<cabac_source>(per_lcu...);
      const u32 want = __builtin_amdgcn_readfirstlane(cb.lcu_ctx ? (u32)cb.lcu_ctx[(size_t)lcu_y * a.lcus_x + lcu_x] : 0u);
      price = { cb.sets + min(want, cb.n_sets - 1u), qp >= cb.fast_limit };   // an index beyond the table is its last set
    }
    if constexpr (RDOQ) {
      // the LCU's context set, state bytes and lambda into LDS once, beside the arrays of the recursion
      __shared__ typename rdoq_lcu<RDOQ>::lds s_rdoq;
      rq.m = &s_rdoq;
      rq.r = source_of<rdoq_source>(per_lcu...);
      rq.qp = qp;
      rq.signhide = q.signhide != 0;
      rq.stage((size_t)lcu_y * a.lcus_x + lcu_x, lane);
    }
  }

  // ---- the walk: 256 SCUs in z-order; a leaf TU is done at its top-left SCU ----
  for (int i = 0; i < 256; ++i) {
    const int ux = compact4(i), uy = compact4(i >> 1);
    tu_pos p;
    p.plane = plane; p.sh = sh;
    p.lx = X0 + 4 * ux; p.ly = Y0 + 4 * uy;
    if (p.lx >= a.width || p.ly >= a.height) continue;
    const size_t scu = (size_t)(p.ly >> 2) * a.cus_stride + (p.lx >> 2);
    // one address for the whole wave: say so, and everything below is scalar
    const u32 head = __builtin_amdgcn_readfirstlane(a.cus[scu * 5]);
    int leaf = 0;
    if (!intra_cu_of(head, p.lx, p.ly, a.width, a.height, p.cu_x, p.cu_y, leaf)) continue;
    if ((p.lx | p.ly) & (leaf - 1)) continue;                                  // inside a TU that was done at its top-left
    int n = leaf;
    if (plane) {
      // chroma TUs are half as wide; with 4x4 luma TUs the chroma of the 8x8 area is one 4x4 TU at its first SCU (transform.c:293-313)
      if (leaf == 4 && ((p.lx | p.ly) & 7)) continue;
      n = leaf > 8 ? leaf >> 1 : 4;
    }
    p.mode = (int)__builtin_amdgcn_readfirstlane((u32)a.modes[2 * scu + (plane ? 1 : 0)]);
    if (p.mode > 34) continue;
    // kvz_get_scan_order (encoderstate.c:1384-1398): luma TUs 8 and 4 wide, chroma TUs 4 wide
    p.scan = (leaf <= 8) ? ((p.mode >= 6 && p.mode <= 14) ? 2 : ((p.mode >= 22 && p.mode <= 30) ? 1 : 0)) : 0;
    p.tx = (p.lx - X0) >> sh; p.ty = (p.ly - Y0) >> sh;
    const quant_consts *kk;
    if constexpr (LCU_QP) kk = own.k;
    else kk = a.k[plane ? 1 : 0];
    if constexpr (RDOQ) {
      // head is the record at the TU's own top-left SCU: the cur_pu of transform.c:437
      const int trd = rq.tr_depth_of(head);
      if (n == 32) intra_tu<32, TILES, SL>(a, p, tr, kk[3], tile, s_ref, s_ext, s_pred, sa, sb, sq, {}, {}, rq, trd);
      else if (n == 16) intra_tu<16, TILES, SL>(a, p, tr, kk[2], tile, s_ref, s_ext, s_pred, sa, sb, sq, {}, {}, rq, trd);
      else if (n == 8) intra_tu<8, TILES, SL>(a, p, tr, kk[1], tile, s_ref, s_ext, s_pred, sa, sb, sq, {}, {}, rq, trd);
      else intra_tu<4, TILES, SL>(a, p, tr, kk[0], tile, s_ref, s_ext, s_pred, sa, sb, sq, {}, {}, rq, trd);
      continue;
    }
    if (n == 32) intra_tu<32, TILES, SL>(a, p, tr, kk[3], tile, s_ref, s_ext, s_pred, sa, sb, sq);
    else if (n == 16) intra_tu<16, TILES, SL>(a, p, tr, kk[2], tile, s_ref, s_ext, s_pred, sa, sb, sq);
    else if (n == 8) intra_tu<8, TILES, SL>(a, p, tr, kk[1], tile, s_ref, s_ext, s_pred, sa, sb, sq);
    else if constexpr (CABAC) intra_tu<4, TILES, SL, TS, true>(a, p, tr, kk[0], tile, s_ref, s_ext, s_pred, sa, sb, sq, skip, price);
    else intra_tu<4, TILES, SL, TS>(a, p, tr, kk[0], tile, s_ref, s_ext, s_pred, sa, sb, sq, skip);
  }

  // ---- the pixels of the intra CUs go back: a row of an SCU (4 luma, 2 chroma pixels) per item, 16 SCUs of a row side by side ----
  const int R = 4 >> sh;
  for (int it = lane; it < 16 * T; it += 64) {
    const int ux = it & 15, r = it >> 4;
    if (!s_intra[(r / R) * 16 + ux]) continue;
    u8 *g = rec + (size_t)(y0 + r) * stride + x0 + R * ux;
    const u8 *l = tile + tpx(R * ux, r);
    if (sh) __builtin_memcpy(g, l, 2);
    else __builtin_memcpy(g, l, 4);
  }
}

// the tile source of a record and its grid; -> false for a malformed grid and for what the one-QP entry refuses
inline bool tile_source_make(const kvz_hip_chain_picture &p, const kvz_hip_tile_grid *grid, tile_source *tiles)
{
  tiles->qp = p.params.qp;
  return chain_one_qp_ok(p) && tile_grid_make(grid, p.src.width, p.src.height, &tiles->grid);
}

// the single-picture entries on their record (chain_picture_pack); per_lcu: nothing (one QP per call, params.qp), or the trailing
// sources of the kernel.  An sl_source among them takes, and requires, params.scaling_list != 0
template <typename... PER_LCU>
int intra_frame(const char *entry, const kvz_hip_chain_picture &p, kvz_hip_stream s, PER_LCU... per_lcu)
{
  if (!chain_picture_args_ok(p, true, pack_has<sl_source, PER_LCU...>)) return kvzhip::invalid_arg(entry);
  const int width = p.src.width, height = p.src.height, chroma = p.params.chroma ? 1 : 0;
  const kvz_hip_quant_params qp = { p.params.qp, p.params.slice_is_intra, p.params.signhide, 0, nullptr, nullptr };
  intra_args a;
  // quant uses type 0 / 2, dequant 0 / 2 / 3 (quant-generic.c:224, :244); flat lists: U and V share their constants.  The shift of
  // the transform depends on the size: a set of constants per size
  __builtin_memset(a.k, 0, sizeof a.k);                                        // not read with a QP array
  for (int i = 0; i < 4 && sizeof...(PER_LCU) == 0; ++i)
    if (!make_consts(&qp, 4 << i, 0, 0, &a.k[0][i]) || !make_consts(&qp, 4 << i, 2, 2, &a.k[1][i])) return kvzhip::invalid_arg(entry);
  a.src[0] = p.src.y; a.src[1] = chroma ? p.src.u : nullptr; a.src[2] = chroma ? p.src.v : nullptr;
  a.rec[0] = p.rec_y; a.rec[1] = chroma ? p.rec_u : nullptr; a.rec[2] = chroma ? p.rec_v : nullptr;
  a.src_stride[0] = p.src.stride_y; a.src_stride[1] = a.src_stride[2] = p.src.stride_c;
  a.rec_stride[0] = p.stride_y; a.rec_stride[1] = a.rec_stride[2] = p.stride_c;
  a.coeff[0] = p.coeff_y; a.coeff[1] = chroma ? p.coeff_u : nullptr; a.coeff[2] = chroma ? p.coeff_v : nullptr;
  a.cus = (u32 *)p.cus; a.modes = p.intra_modes; a.cbf_out = p.cbf_out; a.cost = (u32 *)p.costs;
  a.cus_stride = width >> 2; a.lcus_x = (width + 63) >> 6;
  a.width = width; a.height = height;
  const int lcus_y = (height + 63) >> 6;
  hipStream_t st = ctx_stream(s);
  if (p.cbf_out || p.costs) {
    const int n_scu = (width >> 2) * (height >> 2);
    hipLaunchKernelGGL(intra_recon_init_kernel, dim3((unsigned)((n_scu + 255) / 256)), dim3(256), 0, st, a, n_scu);
    KVZ_CHECK_LAUNCH("intra_recon_init_kernel");
  }
  // the launch sequence depends on width, height and chroma alone
  int waves = a.lcus_x + 2 * (lcus_y - 1), groups = lcus_y;
  if constexpr (sizeof...(PER_LCU) >= 2) {
    // and on the grid: the largest tile's count of waves, a workgroup per LCU row and tile column
    const kvz_hip_tile_grid &g = source_of<tile_source>(per_lcu...).grid;
    waves = tile_grid_waves(g);
    groups = lcus_y * g.cols;
  }
  for (int t = 0; t < waves; ++t) {
    hipLaunchKernelGGL((intra_recon_wave_kernel<intra_args, PER_LCU...>), dim3((unsigned)groups, chroma ? 3u : 1u), dim3(WG), 0, st, a, t, per_lcu...);
    KVZ_CHECK_LAUNCH("intra_recon_wave_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

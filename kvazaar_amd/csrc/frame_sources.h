// frame_sources.h -- what the two residual stages of the picture chain (intra_recon_core.h, inter_residual_core.h) share about
// their options.  A kernel of either stage takes its optional sources as a trailing pack in a fixed order: lcu_qp_source, then the
// stage's own tile_source / sl_source / ts_source (they differ between the stages and live in the cores), then cabac_source; or,
// behind sl_source and without transform skip, rdoq_source.  The
// pack's type selects the instantiation; inside the kernel a source is found by its type (source_of), whatever else the pack holds.
// Also here: the body of the stages' init kernels with the init kernel of the multi-picture entries and its launch.
// Not device code only: the header holds the host code that both stages' record types share and that neither core could hold for the
// other -- rdoq_source_of, the launch of the init kernel, and the fills of the options of a kernel's per-picture record (fill_lists,
// fill_trskip, fill_rdoq, fill_tiles), which is why it includes chain_host.h.  The fill of the picture itself differs between the
// stages and stays beside each core's record.  Everything has internal linkage, as in the cores.
#pragma once

#include "kvz_hip_internal.h"
#include "chain_host.h"

using namespace kvzhip;

namespace {

template <typename T, typename U> struct same_type { static constexpr bool value = false; };
template <typename T> struct same_type<T, T> { static constexpr bool value = true; };
template <typename T, typename... P> constexpr bool pack_has = (same_type<T, P>::value || ...);

// the first T among the arguments; a pack without one does not compile
template <typename T> struct pick {
  template <typename... P> static __host__ __device__ __forceinline__ const T &of(const T &t, const P &...) { return t; }
  template <typename U, typename... P> static __host__ __device__ __forceinline__ const T &of(const U &, const P &...p) { return of(p...); }
};
template <typename T, typename... P> __host__ __device__ __forceinline__ const T &source_of(const P &...p) { return pick<T>::of(p...); }

// A QP per LCU (kvz_hip_inter_residual_frame_qp, kvz_hip_intra_recon_frame_qp): the array and what else the constants depend on, which
// the kernel derives with the function the host uses (flat_consts, quant_core.h).  It is the first trailing argument: without it (one
// QP per call) the instantiation is the kernel as it was.  With a later source the array may be NULL, and that source carries the QP
// of every LCU.
struct lcu_qp_source { const int8_t *lcu_qp; int slice_is_intra, signhide; };
inline lcu_qp_source qp_source_of(const kvz_hip_chain_picture &p) { return { p.lcu_qp, p.params.slice_is_intra ? 1 : 0, p.params.signhide }; }

// CABAC pricing of the two trials of transform skip (kvz_hip_*_frame_ts_cabac) is the last trailing argument, after the transform-skip
// source: the context sets, a set index per LCU (or nullptr: set 0) and cfg.fast_residual_cost_limit.  The rule of rdo.c:214: where
// the QP of the LCU is at or above the limit, the price of a trial is get_coeff_cabac_cost of its 16 levels (coeff_cabac_core.h), below
// it the estimate.
struct cabac_source { const kvz_hip_coeff_ctx *sets; const uint16_t *lcu_ctx; u32 n_sets; int fast_limit; };
// a trial's levels in LDS rows of ld, as coeff_cabac_count reads them
struct cabac_lds_coeffs { const i16 *p; int ld; __device__ __forceinline__ int at(int x, int y) const { return p[y * ld + x]; } };

// RDOQ (kvz_hip_inter_residual_frame_rdoq, kvz_hip_intra_recon_frame_rdoq) is rdoq_source, the last trailing argument, behind the lists
// where there are lists: kvz_hip_rdoq_source as the kernel reads it.  A TU wider than 4, and a 4x4 TU unless skip is set, takes its
// levels from kvz_rdoq (rdoq_core.h through rdoq_stage.h) on the context set and the state of its LCU, an index beyond the table being
// the last set; every other TU keeps the plain quantiser.  What a wave holds about its LCU for that is rdoq_lcu<true>, which
// rdoq_stage.h defines: the translation units without RDOQ never see the cost arithmetic or its floating-point pragma.
struct rdoq_source {
  const kvz_hip_coeff_ctx *sets;
  const kvz_hip_rdoq_state *states;
  const uint16_t *lcu_ctx;
  const int32_t *quant;
  const double *err_scale;
  u32 n_sets;
  int skip;
};
inline rdoq_source rdoq_source_of(const kvz_hip_rdoq_source &r)
{
  return { r.ctx_sets, r.states, r.lcu_ctx, r.tables.quant, r.tables.err_scale, r.n_sets, r.rdoq_skip != 0 };
}
template <bool ON> struct rdoq_lcu { static constexpr bool on = false; };

// The options of a checked record of a multi-picture call into the kernel's per-picture record, which starts as zeros: resid_pic_* and
// intra_pic_* use the same member names on purpose.  The scaling tables (both NULL in a call without them);
template <typename PIC> void fill_lists(PIC &a, const kvz_hip_scaling_tables &t) { a.quant = t.quant; a.dequant = t.dequant; }
// transform skip;
template <typename PIC> void fill_trskip(PIC &a, const kvz_hip_trskip *ts, uint8_t *tr_skip_out)
{
  if (ts) { a.lcu_bit_cost = ts->lcu_bit_cost; a.tr_skip_out = tr_skip_out; a.bit_cost = ts->bit_cost; }
}
// the picture's own part of RDOQ, which every record of a checked call with RDOQ carries;
template <typename PIC> void fill_rdoq(PIC &a, const kvz_hip_rdoq_source &r)
{
  a.sets = r.ctx_sets; a.states = r.states; a.lcu_ctx = r.lcu_ctx; a.n_sets = r.n_sets;
}
// the grid's place in the pool.  The kernel reads cols == 0 as "no grid": a picture without one keeps the zeros, where pic_tiles says
// one tile
template <typename PIC> void fill_tiles(PIC &a, const kvz_hip_tile_grid *grid, const pic_tiles &t)
{
  if (grid) { a.cols = t.cols; a.rows = t.rows; a.col_at = t.col_at; a.row_at = t.row_at; }
}

// The body of the init kernels: outputs that the TUs of several planes accumulate into start from zero inside the stage's CUs, and
// keep their contents elsewhere.  a: the picture's record (cus, cus_stride, cbf_out, cost), i: an SCU of it in raster order, cu_at:
// the stage's CU rule, (a, i, x, y, cu_x, cu_y, leaf) -> whether the SCU at luma (x, y) lies in a CU of the stage, and which.
template <typename PIC, typename CU_RULE>
__device__ __forceinline__ void zero_cu_outputs(const PIC &a, int i, CU_RULE cu_at)
{
  const int sy = i / a.cus_stride, sx = i - sy * a.cus_stride;
  int cu_x, cu_y, leaf;
  if (!cu_at(a, i, 4 * sx, 4 * sy, cu_x, cu_y, leaf)) return;
  if (a.cbf_out) a.cbf_out[i] = 0;
  if (a.cost && cu_x == 4 * sx && cu_y == 4 * sy) {
#pragma unroll
    for (int j = 0; j < 6; ++j) a.cost[(size_t)i * 6 + j] = 0u;
  }
}

// The init kernel of the multi-picture entries, for every picture that has cbf_out or costs: grid (blocks of the largest such picture,
// pictures).  BATCH: the table of per-picture records, CU_RULE: the stage's
template <typename BATCH, typename CU_RULE>
__global__ __launch_bounds__(256) void init_pictures_kernel(BATCH b)
{
  const auto &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  zero_cu_outputs(a, i, CU_RULE());
}
// init_scus: chain_plan's, 0 where no picture has such an output and nothing is launched
template <typename CU_RULE, typename BATCH>
int init_pictures(const BATCH &b, int init_scus, int n_pictures, hipStream_t st)
{
  if (!init_scus) return KVZ_HIP_OK;
  hipLaunchKernelGGL((init_pictures_kernel<BATCH, CU_RULE>), dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
  KVZ_CHECK_LAUNCH("init_pictures_kernel");
  return KVZ_HIP_OK;
}

}  // namespace

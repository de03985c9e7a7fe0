// frame_sources.h -- what the two residual stages of the picture chain (intra_recon_core.h, inter_residual_core.h) share about
// their options.  A kernel of either stage takes its optional sources as a trailing pack in a fixed order: lcu_qp_source, then the
// stage's own tile_source / sl_source / ts_source (they differ between the stages and live in the cores), then cabac_source; or,
// behind sl_source and without transform skip, rdoq_source.  The
// pack's type selects the instantiation; inside the kernel a source is found by its type (source_of), whatever else the pack holds.
// Also here: the body of the stages' init kernels.  Everything has internal linkage, as in the cores.
#pragma once

#include "kvz_hip_internal.h"

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
template <bool ON> struct rdoq_lcu { static constexpr bool on = false; };

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

}  // namespace

// coeff_cost_host.h -- the host side of the CABAC coefficient pricing: what kvz_hip_coeff_cost_batch and the pricing argument of
// the _ts_cabac stages require of their arguments.
// Host only, as chain_host.h is: pointers are compared and never followed, so a plain C++17 compiler takes this header with
// kvz_hip.h alone (tests/test_coeff_cost_abi.py runs it that way).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kvz_hip.h"

namespace {

static_assert(sizeof(kvz_hip_coeff_ctx) == 144 && sizeof(kvz_hip_coeff_cost_desc) == 12 && sizeof(kvz_hip_coeff_cost_params) == 16 &&
              sizeof(kvz_hip_coeff_pricing) == 24, "layout documented in kvz_hip.h");

// kvz_hip_coeff_cost_batch with n > 0: why the call is refused, or nullptr
inline const char *coeff_cost_batch_why(const kvz_hip_coeff *coeffs, const kvz_hip_coeff_cost_desc *descs, size_t n, const kvz_hip_coeff_ctx *ctx_sets,
                                        uint32_t n_sets, const kvz_hip_coeff_cost_params *params, const uint32_t *bits_out)
{
  if (!coeffs || !descs || !ctx_sets || !params || !bits_out) return "a pointer is null";
  if (n_sets == 0) return "n_sets is 0";
  if (n > 0x7fffffffu) return "n above 2^31 - 1";
  if (((uintptr_t)coeffs & 7) || ((uintptr_t)descs & 3) || ((uintptr_t)ctx_sets & 1) || ((uintptr_t)bits_out & 3))
    return "coeffs not 8-byte, descs or bits_out not 4-byte or ctx_sets not 2-byte aligned";
  return nullptr;
}

// the pricing argument of kvz_hip_inter_residual_frame_ts_cabac / kvz_hip_intra_recon_frame_ts_cabac (pricing != NULL)
inline const char *coeff_pricing_why(const kvz_hip_coeff_pricing *pricing, const kvz_hip_trskip *ts)
{
  if (!ts) return "pricing without ts";
  if (!pricing->ctx_sets || ((uintptr_t)pricing->ctx_sets & 1)) return "ctx_sets is null or not 2-byte aligned";
  if (pricing->n_sets == 0) return "n_sets is 0";
  if ((uintptr_t)pricing->lcu_ctx & 1) return "lcu_ctx not 2-byte aligned";
  return nullptr;
}

}  // namespace
